#!/usr/bin/env python3
"""Benchmark of the sparse voxel grid's depth maps (SparseGrid.volume_render_depth_image) on one MI355X.

    python bench_grid_depth.py [--steps 20] [--warmup 3] [--reso 128 256] [--hw 800] [--sigma-thresh 0.0]

The scene of bench_grid.py: the network of bench.py (synthetic_pair(0), 8 x 256, view directions) baked with
SparseGrid.from_nerf(fine, -1.5, 1.5, R), basis_dim 9, after accelerate(), and the 800 x 800 lego camera. Legs, alternated
step by step in one process and timed with HIP events on the current stream after warm-up:
  expected R     grid.volume_render_depth_image(camera)                        the expected termination
  threshold R    grid.volume_render_depth_image(camera, sigma_thresh=x)        the first sample above x
  raylen R       grid.volume_render_image(camera, return_raylen=True)          nothing marched: the floor of a launch
  colour R       grid.volume_render_image(camera)                              the frame the depth has to undercut
Per R also: pixels with depth > 0, and that the depth frame equals the depth of the camera's rays bit for bit. The library
named by NERF_MI355X_LIB is the one measured (an ablation build of nerf-projects_amd/build.py, for the A/B of the pixel
mapping). Prints one JSON line.
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
    p.add_argument("--sigma-thresh", type=float, default=0.0)
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

    grids = {}
    for R in a.reso:
        grids[R] = N.SparseGrid.from_nerf(net_f, -a.box, a.box, R, n_dirs=a.n_dirs)
        grids[R].accelerate()
    legs = {
        "expected": lambda g: g.volume_render_depth_image(cam),
        "threshold": lambda g: g.volume_render_depth_image(cam, sigma_thresh=a.sigma_thresh),
        "raylen": lambda g: g.volume_render_image(cam, return_raylen=True),
        "colour": lambda g: g.volume_render_image(cam),
    }
    times = {R: {leg: [] for leg in legs} for R in a.reso}
    for step in range(a.warmup + a.steps):
        for R in a.reso:
            for leg, fn in legs.items():
                ms, _ = timed(lambda: fn(grids[R]))
                if step >= a.warmup:
                    times[R][leg].append(ms)
    out = {"metric": "grid_depth_frame", "frame": f"lego {H}x{W}, synthetic_pair(0) fine network baked over [-{a.box}, {a.box}], "
           f"basis_dim 9, n_dirs {a.n_dirs}, step_size 0.5, accelerated", "steps": a.steps, "warmup": a.warmup,
           "sigma_thresh": a.sigma_thresh, "library": os.path.basename(_lib.library_path()), "grids": {}}
    rays = cam.gen_rays()
    for R in a.reso:
        g = grids[R]
        assert g.accelerated
        res = {"kept_nodes": g.capacity, "kept_fraction": g.capacity / g.links.numel()}
        for leg in legs:
            res[leg + "_ms"] = float(np.median(times[R][leg]))
            res[leg + "_ms_min"] = float(np.min(times[R][leg]))
            res[leg + "_ms_all"] = times[R][leg]
        for leg, x in (("expected", None), ("threshold", a.sigma_thresh)):
            img = g.volume_render_depth_image(cam, sigma_thresh=x)
            assert torch.equal(img.reshape(-1), g.volume_render_depth(rays, sigma_thresh=x)) and torch.isfinite(img).all()
            res[leg + "_pixels_hit"] = int((img > 0).sum())
        res["pixels"] = H * W
        res["expected_over_colour"] = res["expected_ms"] / res["colour_ms"]
        res["threshold_over_colour"] = res["threshold_ms"] / res["colour_ms"]
        out["grids"][str(R)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
