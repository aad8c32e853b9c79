#!/usr/bin/env python3
"""Benchmark of loss.backward() through the sparse voxel grid's depth and log_transmit (GridModule.volume_render_depth) on
one MI355X.

    python bench_grid_depth_autograd.py [--steps 20] [--warmup 5] [--reso 128 256] [--batch 5000]

The set-up of bench_grid_autograd.py: the fine network of bench.py (synthetic_pair(0), 8 x 256, view directions) baked with
SparseGrid.from_nerf(fine, -1.5, 1.5, R), basis_dim 9, accelerate(); batches of --batch random pixels of the lego camera at
--train-poses azimuths. The depth targets are the grid's own depths times 0.9, the colour targets 0.5 (what the targets
hold changes no kernel's work). Legs, alternated step by step in one process and timed with HIP events on the current
stream after warm-up, median (min - max) reported:
  depth_plain     grid.volume_render_depth(batch, return_log_transmit=True): the plain forward
  depth_taped     m.volume_render_depth(batch, return_log_transmit=True) with grad enabled: the taped forward
  depth_backward  loss.backward() of  mean((depth - target)^2) + 0.1 mean(T (1 - T)),  T = exp(log_transmit): torch's backward
                  of the loss, the zero-fill of the density gradient, the backward kernel with both cotangents
  depth_kernel    nerf_grid_depth_backward alone with both cotangents, on a table zeroed outside the timed region
  depth_step      forward + loss + backward, one timed region
  colour_step     the same for the colour: ((m.volume_render(batch) - 0.5)^2).mean().backward()
Reported per R: depth_step / colour_step (the depth step reads densities only and issues 1 atomic per corner where the colour
step issues 28: it must be below 1) and depth_taped / depth_plain (the tape is one 8-byte store per ray).
Prints one JSON line and writes it to profiles/bench_grid_depth_autograd.json with --write.
"""
import argparse
import ctypes as C
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
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--reso", type=int, nargs="+", default=[128, 256])
    p.add_argument("--batch", type=int, default=5000)
    p.add_argument("--n-dirs", type=int, default=64)
    p.add_argument("--box", type=float, default=1.5)
    p.add_argument("--hw", type=int, default=400)
    p.add_argument("--train-poses", type=float, nargs="+", default=[15.0 * i for i in range(24)])
    p.add_argument("--write", action="store_true")
    a = p.parse_args()
    torch.cuda.set_device(0)
    import nerf_projects_amd as N
    from nerf_projects_amd import _lib, synthetic
    arch = dict(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=4, skips=[4], use_viewdirs=True)
    _, sd_f = synthetic.synthetic_pair(0)
    net_f = N.NeRF(**arch).load_state_dict(sd_f)
    H = W = a.hw
    origins, dirs = [], []
    for theta in a.train_poses:
        K, c2w, _, _ = synthetic.lego_camera(H, W, theta=theta)
        rays = N.Camera.from_nerf_pose(c2w, H, W, float(K[0][0])).gen_rays()
        origins.append(rays.origins)
        dirs.append(rays.dirs)
    origins, dirs = torch.cat(origins), torch.cat(dirs)
    gen = torch.Generator(device="cpu").manual_seed(0)

    def batch():
        k = torch.randint(0, origins.shape[0], (a.batch,), generator=gen).cuda()
        return N.Rays(origins[k].contiguous(), dirs[k].contiguous())

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), r

    def depth_loss(depth, lt, target):
        T = torch.exp(lt)
        return ((depth - target) ** 2).mean() + 0.1 * (T * (1.0 - T)).mean()

    def backward_kernel(g, rays, tape, g_d, g_t, gd):
        b = _lib.GridDepthBackwardArgs()
        b.origins, b.dirs, b.n_rays = rays.origins.data_ptr(), rays.dirs.data_ptr(), rays.origins.shape[0]
        b.grad_depth, b.grad_log_transmit, b.tape, b.grad_density = g_d.data_ptr(), g_t.data_ptr(), tape.data_ptr(), gd.data_ptr()
        b.use_skip, b.stream = 1, g.ctx.stream().value
        _lib.check(g.ctx.lib.nerf_grid_depth_backward(g._handle(), C.byref(g.opt._to_c()), C.byref(b)))

    grids, modules = {}, {}
    for R in a.reso:
        grids[R] = N.SparseGrid.from_nerf(net_f, -a.box, a.box, R, n_dirs=a.n_dirs)
        grids[R].accelerate()
        modules[R] = N.GridModule(grids[R])
    legs = ("depth_plain", "depth_taped", "depth_backward", "depth_kernel", "depth_step", "colour_step")
    t = {R: {leg: [] for leg in legs} for R in a.reso}
    for step in range(a.warmup + a.steps):
        rays = batch()
        for R in a.reso:
            g, m = grids[R], modules[R]
            ms = {}
            ms["depth_plain"], (ref, ref_lt) = timed(lambda: g.volume_render_depth(rays, return_log_transmit=True))
            target = ref * 0.9
            m.zero_grad(set_to_none=True)
            ms["depth_taped"], (depth, lt) = timed(lambda: m.volume_render_depth(rays, return_log_transmit=True))
            assert torch.equal(depth, ref) and torch.equal(lt, ref_lt)
            tape = depth.grad_fn.saved_tensors[3]      # (before the backward frees it)
            d_leaf, t_leaf = depth.detach().requires_grad_(True), lt.detach().requires_grad_(True)
            depth_loss(d_leaf, t_leaf, target).backward()      # the cotangents torch will hand to the kernel
            ms["depth_backward"], _ = timed(depth_loss(depth, lt, target).backward)
            gd = torch.zeros_like(g.density_data)
            ms["depth_kernel"], _ = timed(lambda: backward_kernel(g, rays, tape, d_leaf.grad.contiguous(), t_leaf.grad.contiguous(), gd))
            assert float((gd - m.density_data.grad).abs().max()) <= 1e-4 * float(gd.abs().max()) and float(gd.abs().max()) > 0
            assert m.sh_data.grad is None
            m.zero_grad(set_to_none=True)
            ms["depth_step"], _ = timed(lambda: depth_loss(*m.volume_render_depth(rays, return_log_transmit=True), target).backward())
            m.zero_grad(set_to_none=True)
            ms["colour_step"], _ = timed(lambda: ((m.volume_render(rays) - 0.5) ** 2).mean().backward())
            m.zero_grad(set_to_none=True)
            if step >= a.warmup:
                for leg in legs:
                    t[R][leg].append(ms[leg])
    out = {"metric": "grid_depth_autograd", "setup": f"synthetic_pair(0) fine network baked over [-{a.box}, {a.box}], basis_dim 9, "
           f"n_dirs {a.n_dirs}, accelerated; batches of {a.batch} random rays of {len(a.train_poses)} lego poses at {H}x{W}",
           "steps": a.steps, "warmup": a.warmup, "grids": {}}
    for R in a.reso:
        g = grids[R]
        med = {leg: float(np.median(t[R][leg])) for leg in legs}
        out["grids"][str(R)] = {
            "kept_nodes": g.capacity, "ms": med, "ms_min": {leg: float(np.min(t[R][leg])) for leg in legs},
            "ms_max": {leg: float(np.max(t[R][leg])) for leg in legs}, "ms_all": t[R],
            "depth_step_over_colour_step": med["depth_step"] / med["colour_step"],
            "depth_taped_over_depth_plain": med["depth_taped"] / med["depth_plain"],
            "depth_rays_per_s": a.batch * 1e3 / med["depth_step"],
        }
    line = json.dumps(out)
    print(line)
    if a.write:
        with open(os.path.join(ROOT, "profiles", "bench_grid_depth_autograd.json"), "w") as f:
            f.write(line + "\n")
    slow = [R for R in a.reso if out["grids"][str(R)]["depth_step_over_colour_step"] >= 1.0]
    if slow:
        sys.exit(f"the depth step is not faster than the colour step at R = {slow}")


if __name__ == "__main__":
    main()
