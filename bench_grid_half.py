#!/usr/bin/env python3
"""Benchmark of the half-precision sparse voxel grid (HalfGrid) against the fp32 grid it was made from, on one MI355X.

    python bench_grid_half.py [--steps 20] [--warmup 3] [--reso 128 256] [--hw 800]

The scene of bench_grid.py: the network of bench.py (synthetic_pair(0), 8 x 256, view directions) baked with
SparseGrid.from_nerf(fine, -1.5, 1.5, R), basis_dim 9, and the 800 x 800 lego camera. Legs, alternated step by step in one
process and timed with HIP events on the current stream after warm-up, each once on the plain grid and once after accelerate():
  float R        SparseGrid.volume_render_image(camera)                         the fp32 table, 108 B per row
  single R       HalfGrid(lanes="single").volume_render_image(camera)           64 B per row, one coefficient per lane
  pair R         HalfGrid(lanes="pair").volume_render_image(camera)             64 B per row, two coefficients per lane
  default R      HalfGrid().volume_render_image(camera)                         the mapping the library ships as its default
Per R also: the bytes of both colour tables, the PSNR of the half frame against the fp32 frame (finite only because a bake is
not fp16-exact), and the check that the half frame IS the fp32 frame of the widened table (to_float()), bit for bit, in both
mappings - which is what a grid loaded from a checkpoint gets. Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reso", type=int, nargs="+", default=[128, 256])
    p.add_argument("--n-dirs", type=int, default=64)
    p.add_argument("--box", type=float, default=1.5)
    p.add_argument("--hw", type=int, default=800)
    a = p.parse_args()
    if a.steps < 1 or a.warmup < 0:
        p.error("--steps >= 1 and --warmup >= 0 are required")
    torch.cuda.set_device(0)
    import nerf_projects_amd as N
    from nerf_projects_amd import _lib, synthetic
    arch = dict(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=4, skips=[4], use_viewdirs=True)
    _, sd_f = synthetic.synthetic_pair(0)
    net_f = N.NeRF(**arch).load_state_dict(sd_f)
    H = W = a.hw
    K, c2w, _, _ = synthetic.lego_camera(H, W)
    cam = N.Camera.from_nerf_pose(c2w, H, W, float(K[0][0]))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), r

    legs = ("float", "single", "pair", "default")
    out = {"metric": "grid_half_frame", "frame": f"lego {H}x{W}, synthetic_pair(0) fine network baked over [-{a.box}, {a.box}], "
           f"basis_dim 9, n_dirs {a.n_dirs}, step_size 0.5", "steps": a.steps, "warmup": a.warmup,
           "library": os.path.basename(_lib.library_path()), "grids": {}}
    for R in a.reso:
        grids = {"float": N.SparseGrid.from_nerf(net_f, -a.box, a.box, R, n_dirs=a.n_dirs)}
        for lanes in ("single", "pair", None):
            grids[lanes or "default"] = grids["float"].to_half(lanes=lanes)
        res = {"kept_nodes": grids["float"].capacity, "kept_fraction": grids["float"].capacity / grids["float"].links.numel(),
               "float_sh_bytes": grids["float"].sh_data.numel() * 4, "half_sh_bytes": grids["default"].sh_bytes}
        res["sh_bytes_ratio"] = res["half_sh_bytes"] / max(1, res["float_sh_bytes"])
        for mode in ("plain", "accelerated"):
            if mode == "accelerated":
                for g in grids.values():
                    g.accelerate()
            times = {leg: [] for leg in legs}
            for step in range(a.warmup + a.steps):
                for leg in legs:
                    ms, _ = timed(lambda: grids[leg].volume_render_image(cam))
                    if step >= a.warmup:
                        times[leg].append(ms)
            for leg in legs:
                res[f"{mode}_{leg}_ms"] = float(np.median(times[leg]))
                res[f"{mode}_{leg}_ms_min"] = float(np.min(times[leg]))
                res[f"{mode}_{leg}_ms_all"] = times[leg]
            for leg in legs[1:]:
                res[f"{mode}_{leg}_over_float"] = res[f"{mode}_{leg}_ms"] / res[f"{mode}_float_ms"]
            res[f"{mode}_pair_over_single"] = res[f"{mode}_pair_ms"] / res[f"{mode}_single_ms"]
        ref = grids["float"].volume_render_image(cam)
        widened = grids["default"].to_float()
        widened.accelerate()
        exact = widened.volume_render_image(cam)
        for leg in legs[1:]:
            assert torch.equal(grids[leg].volume_render_image(cam), exact), leg      # lossless on the table it holds
        mse = float(((exact.double() - ref.double()) ** 2).mean())
        res["psnr_half_vs_float_db"] = float("inf") if mse == 0.0 else float(-10.0 * np.log10(mse))
        res["max_abs_half_vs_float"] = float((exact - ref).abs().max())
        res["pixels"] = H * W
        out["grids"][str(R)] = res
        del grids, widened
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
