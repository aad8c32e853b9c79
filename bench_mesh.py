#!/usr/bin/env python3
"""Benchmark of mesh extraction (gen_mesh.marching_cubes, nerf-projects_amd/mesh.py) on one MI355X.

    python bench_mesh.py [--steps 5] [--warmup 2] [--reso 256 300]

Network: the bench network (synthetic_pair(0)'s fine net, 8 x 256 with view directions), lattice [-1.1, 1.1]^3 at R^3
nodes, iso = the median of the positive sigma on a 64^3 lattice of the same box. Per R, timed with HIP events on the
current stream after warm-up, the legs alternated step by step in one process:
  lattice        density_grid: the fused kernel on lattice nodes (sigma only) - points/s, TFLOP/s (1,186,816 FLOP per
                 point: the kernel runs the whole chain) and the share of the roof bench.py prices the frame kernel with
                 (f16x2: 2516.6 / 3 TFLOP/s; f32: 157.3)
  run_network    the same lattice materialised as [N, 1, 3] points (+ one view direction per point) through run_network:
                 the baseline a user had without density_grid (the points are made outside the timed region)
  marching_cubes marching_cubes_volume on the lattice's sigma: time (both of its calls: count, then count + emit; each
                 synchronises), the compulsory bytes (volume read once, vertices and triangles written) per second against
                 the 6.0 TB/s read ceiling (profiles/microbench), its share of the lattice time
Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FLOP_PER_EVAL = 1186816
PEAK_FP32_MFMA_TFLOPS = 157.3
PEAK_FP16_MFMA_TFLOPS = 2516.6
READ_CEILING_TB_S = 6.0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--reso", type=int, nargs="+", default=[256, 300])
    p.add_argument("--precision", default="f16x2", choices=["f16x2", "f32"])
    a = p.parse_args()
    torch.cuda.set_device(0)
    import nerf_projects_amd as N
    from nerf_projects_amd import synthetic
    ctx = N.get_context()
    ctx.set_precision(a.precision)
    arch = dict(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=4, skips=[4], use_viewdirs=True)
    net = N.NeRF(**arch).load_state_dict(synthetic.synthetic_pair(0)[1])
    q = N.make_network_query_fn(N.get_embedder(10, 0)[0], N.get_embedder(4, 0)[0])
    c1, c2 = -1.1, 1.1
    s64 = N.density_grid(net, c1, c2, 64)
    iso = float(s64[s64 > 0].median())
    peak = PEAK_FP16_MFMA_TFLOPS / 3 if a.precision == "f16x2" else PEAK_FP32_MFMA_TFLOPS
    out = {"metric": "mesh_extraction", "network": "synthetic_pair(0) fine, 8x256, viewdirs", "box": [c1, c2],
           "iso": iso, "precision": a.precision, "roof_tflops": peak, "steps": a.steps, "warmup": a.warmup, "reso": {}}
    for R in a.reso:
        P = R ** 3
        # the lattice as gen_mesh materialises it (np.linspace -> fp32), for the run_network baseline
        ax = torch.as_tensor(np.linspace(c1, c2, R, dtype=np.float32))
        pts = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 1, 3).cuda()
        vd = torch.nn.functional.normalize(torch.ones((P, 3), device="cuda"), dim=-1)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        t_grid, t_rn, t_mc = [], [], []
        for step in range(a.warmup + a.steps):
            ev[0].record()
            sigma = N.density_grid(net, c1, c2, R)
            ev[1].record()
            ev[2].record()
            raw = q(pts, vd, net)
            ev[3].record()
            del raw
            ev[4].record()
            v, t = N.marching_cubes_volume(sigma, iso)
            ev[5].record()
            torch.cuda.synchronize()
            if step >= a.warmup:
                t_grid.append(ev[0].elapsed_time(ev[1]))
                t_rn.append(ev[2].elapsed_time(ev[3]))
                t_mc.append(ev[4].elapsed_time(ev[5]))
        nv, nt = int(v.shape[0]), int(t.shape[0])
        g, r, m = float(np.median(t_grid)), float(np.median(t_rn)), float(np.median(t_mc))
        tf = P * FLOP_PER_EVAL / (g * 1e-3) / 1e12
        mc_bytes = 4 * P + 12 * nv + 24 * nt
        out["reso"][str(R)] = {
            "points": P,
            "lattice": {"ms": g, "ms_all": t_grid, "points_per_s": P / (g * 1e-3), "tflops": tf, "frac_of_roof": tf / peak},
            "run_network_baseline": {"ms": r, "ms_all": t_rn, "points_per_s": P / (r * 1e-3),
                                     "tflops": P * FLOP_PER_EVAL / (r * 1e-3) / 1e12, "lattice_speedup": r / g},
            "marching_cubes": {"ms": m, "ms_all": t_mc, "compulsory_bytes": mc_bytes,
                               "tb_per_s": mc_bytes / (m * 1e-3) / 1e12,
                               "frac_of_read_ceiling": mc_bytes / (m * 1e-3) / 1e12 / READ_CEILING_TB_S,
                               "share_of_lattice_time": m / g},
            "n_vertices": nv, "n_triangles": nt,
        }
        del pts, vd, sigma, v, t
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
