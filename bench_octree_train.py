#!/usr/bin/env python3
"""Benchmark of PlenOctree fine-tuning (N3Tree.mse_backward, csrc/octree_grad_kernels.hip) on one MI355X.

    python bench_octree_train.py [--steps 20] [--warmup 3] [--reso 128 256] [--hw 800] [--ab]

The scene of bench_octree.py: the network of bench.py baked with SparseGrid.from_nerf(fine, -1.5, 1.5, R), basis_dim 9, the
800 x 800 lego camera, the tree N3Tree.from_grid of that grid; the target is a seeded random image. Legs, alternated step by
step in one process (in reversed order on every other step) and timed with HIP events; a leg is --reps frames enqueued back to
back between one pair of events, divided by --reps:
  forward R            tree.volume_render_image(camera, step_size=1e-3)          the parent's frame (profiles/octree.md)
  mse_backward R       tree.mse_backward(camera, target, step_size=1e-3)          two marches and the scatter, one launch
  mse_backward_table R the same after tree.accelerate(--levels)
  zero_update R        grad.zero_(); data.add_(grad, alpha=-lr)                   the torch ops of a step, over all of data
  scatter_wave / scatter_lane R (--ab)  mse_backward with NERF_OCTREE_SCATTER=wave / lane: the two scatter mappings. Needs a
                       library built with profiles/microbench/octree_lane_scatter.patch applied (the shipped library has the
                       wave flush alone and does not read the variable).
Per R also: shaded leaves per ray (the numpy oracle's march on every --sample-th pixel), the bytes of float atomics per frame
they imply (D floats a shaded leaf; adds of exact zeros are skipped, so an upper bound) and those bytes / the mse_backward
frame, to set against the 1.3 TB/s at which well-shaped float atomics run. The library named by NERF_MI355X_LIB is the one
measured. Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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
    p.add_argument("--sample", type=int, default=97, help="every n-th pixel goes through the numpy march")
    p.add_argument("--ab", action="store_true", help="also time the two scatter mappings (needs the patched library)")
    a = p.parse_args()
    if a.steps < 1 or a.warmup < 0:
        p.error("--steps >= 1 and --warmup >= 0 are required")
    torch.cuda.set_device(0)
    import nerf_projects_amd as N
    from nerf_projects_amd import _lib, synthetic
    import octree_grad_oracle as G
    arch = dict(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=4, skips=[4], use_viewdirs=True)
    _, sd_f = synthetic.synthetic_pair(0)
    net_f = N.NeRF(**arch).load_state_dict(sd_f)
    H = W = a.hw
    K, c2w, _, _ = synthetic.lego_camera(H, W)
    cam = N.Camera.from_nerf_pose(c2w, H, W, float(K[0][0]))
    target = torch.rand(H, W, 3, device="cuda", generator=torch.Generator("cuda").manual_seed(0))

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    trees, tabled = {}, {}
    for R in a.reso:
        grid = N.SparseGrid.from_nerf(net_f, -a.box, a.box, R, n_dirs=a.n_dirs)
        trees[R] = N.N3Tree.from_grid(grid)
        trees[R].data.grad = torch.zeros_like(trees[R].data)
        tabled[R] = trees[R].to(trees[R].device)      # the same arrays (and gradient) behind a handle that gets the table
        tabled[R].accelerate(a.levels)
        del grid

    def scatter(mapping):
        def f(R):
            os.environ["NERF_OCTREE_SCATTER"] = mapping
            trees[R].mse_backward(cam, target, step_size=1e-3)
        return f

    def zero_update(R):
        t = trees[R]
        t.data.grad.zero_()
        t.data.add_(t.data.grad, alpha=-0.0)      # (the gradient is zero: data keeps its bits, the traffic is a step's)

    legs = {
        "forward": lambda R: trees[R].volume_render_image(cam, step_size=1e-3),
        "mse_backward": lambda R: trees[R].mse_backward(cam, target, step_size=1e-3),
        "mse_backward_table": lambda R: tabled[R].mse_backward(cam, target, step_size=1e-3),
        "zero_update": zero_update,
    }
    if a.ab:
        legs["scatter_wave"] = scatter("wave")
        legs["scatter_lane"] = scatter("lane")
    times = {R: {leg: [] for leg in legs} for R in a.reso}
    for step in range(a.warmup + a.steps):
        for R in a.reso:
            for leg, fn in (list(legs.items()) if step % 2 == 0 else list(legs.items())[::-1]):
                ms = timed(lambda: fn(R), a.reps)
                os.environ.pop("NERF_OCTREE_SCATTER", None)
                if step >= a.warmup:
                    times[R][leg].append(ms)
            trees[R].data.grad.zero_()      # (the legs add into it: keep it finite over a long run)
    out = {"metric": "octree_train_frame", "frame": f"lego {H}x{W}, synthetic_pair(0) fine network baked over [-{a.box}, {a.box}], "
           f"basis_dim 9, n_dirs {a.n_dirs}, random target", "steps": a.steps, "warmup": a.warmup, "reps": a.reps,
           "library": os.path.basename(_lib.library_path()), "atomic_rate_guide_TBps": 1.3, "trees": {}}
    rays = cam.gen_rays()
    for R in a.reso:
        t = trees[R]
        res = {"nodes": t.n_internal, "data_bytes": t.data.numel() * 4, "max_depth": t.max_depth, "table_levels": tabled[R].table_levels}
        for leg in times[R]:
            v = times[R][leg]
            res[leg + "_ms"] = float(np.median(v))
            res[leg + "_ms_min"] = float(np.min(v))
            res[leg + "_ms_spread"] = float(np.max(v) - np.min(v))
        # the fused form against torch on the same frame: loss, and the gradient's largest difference relative to its largest entry
        t.data.grad.zero_()
        loss = t.mse_backward(cam, target, step_size=1e-3)
        fused = t.data.grad.clone()
        t.data.grad = None
        t.requires_grad_()
        mse = ((t.volume_render_image(cam, step_size=1e-3).clamp(0.0, 1.0) - target) ** 2).mean()
        mse.backward()
        res["loss"], res["loss_torch"] = float(loss), float(mse.detach())
        res["grad_max"] = float(fused.abs().max())
        res["grad_max_diff_to_autograd"] = float((fused - t.data.grad).abs().max())
        res["rows_touched"] = int((fused.reshape(-1, t.data_dim) != 0).any(1).sum())
        t.requires_grad_(False)
        t.data.grad = None
        del fused
        # shaded leaves per ray: the numpy march on a subsample of the frame's rays
        idx = torch.arange(0, H * W, a.sample, device="cuda")
        tree_np = {"child": t.child.cpu().numpy(), "data": t.data.detach().cpu().numpy(), "invradius": t.invradius.numpy(),
                   "offset": t.offset.numpy(), "rgb_activation": t.rgb_activation, "max_depth": t.max_depth}
        _, steps, lv, _ = G.march(tree_np, rays.origins[idx].cpu().numpy(), rays.dirs[idx].cpu().numpy(), step_size=1e-3)
        sigma = tree_np["data"].reshape(-1, t.data_dim)[:, -1]
        shaded = ((lv >= 0) & (sigma[np.maximum(lv, 0)] > 0)).sum(1)
        res["sampled_rays"] = int(idx.numel())
        res["leaves_per_ray"] = float(steps.mean())
        res["shaded_leaves_per_ray"] = float(shaded.mean())
        res["atomic_bytes_per_frame"] = float(shaded.mean()) * H * W * t.data_dim * 4
        res["atomic_TBps_over_backward_frame"] = res["atomic_bytes_per_frame"] / (res["mse_backward_ms"] * 1e-3) / 1e12
        res["backward_over_forward"] = res["mse_backward_ms"] / res["forward_ms"]
        res["zero_update_over_backward"] = res["zero_update_ms"] / res["mse_backward_ms"]
        res["capped_rays"] = t.capped_rays()
        res["pixels"] = H * W
        out["trees"][str(R)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
