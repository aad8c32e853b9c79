#!/usr/bin/env python3
"""Benchmark of the sparse voxel grid renderer (nerf-projects_amd/grid.py) on one MI355X.

    python bench_grid.py [--steps 5] [--warmup 2] [--reso 128 256] [--n-dirs 64] [--hw 800]

The network of bench.py (synthetic_pair(0), 8 x 256, view directions) baked with SparseGrid.from_nerf(fine, -1.5, 1.5, R),
basis_dim 9, and the 800 x 800 lego camera. Legs, alternated step by step in one process and timed with HIP events on the
current stream after warm-up:
  plain R        grid.volume_render_image(camera) without skip data
  accelerated R  the same after grid.accelerate()
  occupancy      render(..., occupancy=OccupancyGrid.build([coarse, fine], -1.5, 1.5, 97, dilate=2, outside="empty")): the
                 network renderer this one has to beat (the grid of profiles/bench_sparse.json)
Per R: bake time (one run, it synchronises), kept fraction, bytes of the grid, accelerate() time, samples whose links were
loaded and samples shaded per ray (from an instrumented launch of its own, not a timed one), the compulsory bytes
  shaded x 8 x (4 + 4 + 108) B of links, densities and SH rows + (visited - shaded) x 8 x (4 + 4) B
and the rate they imply, PSNR and pixels off by more than 1e-2 against the dense network render of the same camera (this
measures the representation, not the kernel). Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--reso", type=int, nargs="+", default=[128, 256])
    p.add_argument("--n-dirs", type=int, default=64)
    p.add_argument("--box", type=float, default=1.5)
    p.add_argument("--hw", type=int, default=800)
    p.add_argument("--occ-reso", type=int, default=97)
    a = p.parse_args()
    torch.cuda.set_device(0)
    import nerf_projects_amd as N
    from nerf_projects_amd import synthetic
    arch = dict(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=4, skips=[4], use_viewdirs=True)
    sd_c, sd_f = synthetic.synthetic_pair(0)
    net_c, net_f = N.NeRF(**arch).load_state_dict(sd_c), N.NeRF(**arch).load_state_dict(sd_f)
    q = N.make_network_query_fn(N.get_embedder(10, 0)[0], N.get_embedder(4, 0)[0])
    H = W = a.hw
    K, c2w, near, far = synthetic.lego_camera(H, W)
    kw = dict(chunk=32768, c2w=c2w, ndc=False, near=near, far=far, use_viewdirs=True, network_fn=net_c, network_fine=net_f,
              network_query_fn=q, N_samples=64, N_importance=128, white_bkgd=True, perturb=0., raw_noise_std=0.)
    cam = N.Camera.from_nerf_pose(c2w, H, W, float(K[0][0]))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), r

    plain, accel, bake_s, accel_ms = {}, {}, {}, {}
    for R in a.reso:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plain[R] = N.SparseGrid.from_nerf(net_f, -a.box, a.box, R, n_dirs=a.n_dirs)
        torch.cuda.synchronize()
        bake_s[R] = time.perf_counter() - t0
        g = plain[R]
        accel[R] = N.SparseGrid.from_tensors(g.links, g.density_data, g.sh_data, g.radius, g.center)
        accel[R].opt = g.opt
        accel[R].accelerate()
        accel_ms[R] = []
    occ = N.OccupancyGrid.build([net_c, net_f], -a.box, a.box, a.occ_reso, dilate=2, outside="empty")
    t_plain, t_accel, t_occ = {R: [] for R in a.reso}, {R: [] for R in a.reso}, []
    for step in range(a.warmup + a.steps):
        keep = step >= a.warmup
        ms, _ = timed(lambda: N.render(H, W, K, occupancy=occ, **kw)[0])
        if keep:
            t_occ.append(ms)
        for R in a.reso:
            ms, _ = timed(lambda: plain[R].volume_render_image(cam))
            if keep:
                t_plain[R].append(ms)
            ms, _ = timed(lambda: accel[R].volume_render_image(cam))
            if keep:
                t_accel[R].append(ms)
            ms, _ = timed(lambda: accel[R].accelerate())
            if keep:
                accel_ms[R].append(ms)
    dense = N.render(H, W, K, **kw)[0]
    tocc = float(np.median(t_occ))
    out = {"metric": "grid_frame", "frame": f"lego {H}x{W}, synthetic_pair(0) fine network baked over [-{a.box}, {a.box}], basis_dim 9, "
           f"n_dirs {a.n_dirs}, step_size 0.5, white background", "steps": a.steps, "warmup": a.warmup,
           "occupancy_render": {"reso": a.occ_reso, "ms": tocc, "ms_all": t_occ}, "grids": {}}
    n_rays = H * W
    for R in a.reso:
        g = accel[R]
        img = g.volume_render_image(cam)
        assert torch.equal(img, plain[R].volume_render_image(cam))
        v_a, s_a = g.count_samples(camera=cam)
        v_p, s_p = plain[R].count_samples(camera=cam)
        d = (img - dense).abs().reshape(-1, 3).max(-1).values
        mse = float(((img - dense).double() ** 2).mean())
        tp, ta = float(np.median(t_plain[R])), float(np.median(t_accel[R]))
        grid_bytes = g.links.numel() * 4 + g.density_data.numel() * 4 + g.sh_data.numel() * 4

        def compulsory(v, s):
            return s * 8 * (4 + 4 + 108) + (v - s) * 8 * (4 + 4)
        out["grids"][str(R)] = {
            "bake_s": bake_s[R], "kept_nodes": g.capacity, "kept_fraction": g.capacity / g.links.numel(), "grid_bytes": grid_bytes,
            "skip_bytes": g.links.numel(), "accelerate_ms": float(np.median(accel_ms[R])),
            "plain_ms": tp, "plain_ms_all": t_plain[R], "accelerated_ms": ta, "accelerated_ms_all": t_accel[R],
            "visited_per_ray_plain": v_p / n_rays, "visited_per_ray_accelerated": v_a / n_rays, "shaded_per_ray": s_a / n_rays,
            "shaded_equal_plain_accelerated": bool(s_a == s_p),
            "compulsory_bytes_plain": compulsory(v_p, s_p), "compulsory_bytes_accelerated": compulsory(v_a, s_a),
            "compulsory_TBps_plain": compulsory(v_p, s_p) / (tp * 1e-3) / 1e12,
            "compulsory_TBps_accelerated": compulsory(v_a, s_a) / (ta * 1e-3) / 1e12,
            "speedup_over_occupancy_render": tocc / ta, "faster_than_occupancy_render": bool(ta < tocc),
            "psnr_vs_dense_network_db": float(-10.0 * np.log10(max(mse, 1e-30))),
            "pixels_over_1e-2": int((d > 1e-2).sum()), "pixels": int(d.numel()),
        }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
