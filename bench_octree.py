#!/usr/bin/env python3
"""Benchmark of the PlenOctree renderer (N3Tree.volume_render_image) and of N3Tree.from_grid on one MI355X.

    python bench_octree.py [--steps 20] [--warmup 3] [--reso 128 256] [--hw 800]

The scene of bench_grid.py: the network of bench.py (synthetic_pair(0), 8 x 256, view directions) baked with
SparseGrid.from_nerf(fine, -1.5, 1.5, R), basis_dim 9, and the 800 x 800 lego camera; the tree is N3Tree.from_grid of that
grid. Legs, alternated step by step in one process (in reversed order on every other step, so that no leg always follows
the same one) and timed with HIP events on the current stream after warm-up. An octree frame is well under a millisecond, less
than a few calls' host work, so an octree leg is --reps frames enqueued back to back between one pair of events, divided by
--reps: the device is never idle between them and the host's share is not in the figure:
  octree R step  tree.volume_render_image(camera, step_size=1e-3 | 1e-5)     the octree frame, descents from the root
  table R step   the same after tree.accelerate(--levels)                    descents from the table
  grid R         grid.volume_render_image(camera)                            the trilinear frame of the grid it came from
                                                                             (step_size 0.5 voxels, accelerated)
  build R        N3Tree.from_grid(grid)                                      the whole build, its one wait included
Per R also: nodes, leaves, bytes, mean leaves visited per ray, ns per visited leaf, and that the frame equals the render of
the camera's rays bit for bit. The library named by NERF_MI355X_LIB is the one measured. Prints one JSON line.
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
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reso", type=int, nargs="+", default=[128, 256])
    p.add_argument("--n-dirs", type=int, default=64)
    p.add_argument("--box", type=float, default=1.5)
    p.add_argument("--hw", type=int, default=800)
    p.add_argument("--reps", type=int, default=8)
    p.add_argument("--levels", type=int, default=6)
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

    def timed(fn, reps=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps, r

    grids, trees, tabled = {}, {}, {}
    for R in a.reso:
        grids[R] = N.SparseGrid.from_nerf(net_f, -a.box, a.box, R, n_dirs=a.n_dirs)
        grids[R].accelerate()
        trees[R] = N.N3Tree.from_grid(grids[R])
        tabled[R] = trees[R].to(trees[R].device)      # the same arrays behind a handle of its own, which gets the table
        tabled[R].accelerate(a.levels)
    legs = {
        "octree_1e-3": lambda R: trees[R].volume_render_image(cam, step_size=1e-3),
        "octree_1e-5": lambda R: trees[R].volume_render_image(cam, step_size=1e-5),
        "table_1e-3": lambda R: tabled[R].volume_render_image(cam, step_size=1e-3),
        "table_1e-5": lambda R: tabled[R].volume_render_image(cam, step_size=1e-5),
        "grid": lambda R: grids[R].volume_render_image(cam),
    }
    times = {R: {leg: [] for leg in list(legs) + ["build"]} for R in a.reso}
    for step in range(a.warmup + a.steps):
        for R in a.reso:
            for leg, fn in (list(legs.items()) if step % 2 == 0 else list(legs.items())[::-1]):
                ms, _ = timed(lambda: fn(R), 1 if leg == "grid" else a.reps)
                if step >= a.warmup:
                    times[R][leg].append(ms)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            N.N3Tree.from_grid(grids[R])
            torch.cuda.synchronize()
            if step >= a.warmup:
                times[R]["build"].append((time.perf_counter() - t0) * 1e3)
    out = {"metric": "octree_frame", "frame": f"lego {H}x{W}, synthetic_pair(0) fine network baked over [-{a.box}, {a.box}], "
           f"basis_dim 9, n_dirs {a.n_dirs}", "steps": a.steps, "warmup": a.warmup, "reps": a.reps,
           "library": os.path.basename(_lib.library_path()), "trees": {}}
    rays = cam.gen_rays()
    for R in a.reso:
        g, t = grids[R], trees[R]
        res = {"kept_nodes": g.capacity, "nodes": t.n_internal, "leaves": t.n_leaves, "bytes": t.nbytes(), "max_depth": t.max_depth,
               "table_levels": tabled[R].table_levels, "table_bytes": 8 << (3 * tabled[R].table_levels)}
        for leg in times[R]:
            v = times[R][leg]
            res[leg + "_ms"] = float(np.median(v))
            res[leg + "_ms_min"] = float(np.min(v))
            res[leg + "_ms_spread"] = float(np.max(v) - np.min(v))
        for step_size in (1e-3, 1e-5):
            tag = f"octree_{step_size:g}".replace("0.001", "1e-3").replace("1e-05", "1e-5")
            img, steps = t.volume_render_image(cam, step_size=step_size, return_steps=True)
            rgb, rsteps = t.volume_render(rays, step_size=step_size, return_steps=True)
            assert torch.equal(img.reshape(-1, 3), rgb) and torch.equal(steps.reshape(-1), rsteps) and torch.isfinite(img).all()
            timg, tsteps = tabled[R].volume_render_image(cam, step_size=step_size, return_steps=True)
            assert torch.equal(timg, img) and torch.equal(tsteps, steps)      # the table changes no bit
            visited = int(steps.sum())
            res[tag + "_mean_steps"] = visited / (H * W)
            res[tag + "_ns_per_leaf"] = res[tag + "_ms"] * 1e6 / max(visited, 1)
        res["capped_rays"] = t.capped_rays()
        res["table_over_octree_1e-3"] = res["table_1e-3_ms"] / res["octree_1e-3_ms"]
        res["table_over_octree_1e-5"] = res["table_1e-5_ms"] / res["octree_1e-5_ms"]
        res["octree_over_grid"] = res["octree_1e-3_ms"] / res["grid_ms"]
        res["pixels"] = H * W
        out["trees"][str(R)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
