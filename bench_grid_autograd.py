#!/usr/bin/env python3
"""Benchmark of loss.backward() through the sparse voxel grid (nerf-projects_amd/grid_autograd.py) on one MI355X.

    python bench_grid_autograd.py [--steps 20] [--warmup 5] [--reso 128 256] [--batch 5000] [--points 1000000]

The set-up of bench_grid_train.py: the network of bench.py (synthetic_pair(0), 8 x 256, view directions) baked with
SparseGrid.from_nerf(fine, -1.5, 1.5, R), basis_dim 9, accelerate(); batches of --batch random pixels of the lego camera at
--train-poses azimuths, the targets the network's own render(). Legs, alternated step by step in one process and timed with
HIP events on the current stream after warm-up, median (min - max) reported:
  render            grid.volume_render(batch): the yardstick
  forward_backward  GridTrainer.forward_backward(batch, targets): the fused kernel (gradients zeroed outside the timed region)
  ag_forward        m.volume_render(batch) with grad enabled: the taped render
  ag_backward       loss.backward() of the MSE: torch's backward of the loss, the zero-fill of both gradient tables, the
                    backward kernel, and autograd handing the tables to .grad (.grad is None before: no accumulation add)
  ag_kernel         nerf_grid_render_backward alone, on tables zeroed outside the timed region
  ag_step           forward + loss + backward, one timed region
  sample_forward / sample_backward  m.sample on --points random points inside the box, and backward of a weighted sum
Reported per R: ag_step / forward_backward, and (ag_forward + ag_kernel) / forward_backward, the kernel part alone.
Prints one JSON line and writes it to profiles/bench_grid_autograd.json with --write.
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
    p.add_argument("--points", type=int, default=1000000)
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
    sd_c, sd_f = synthetic.synthetic_pair(0)
    net_c, net_f = N.NeRF(**arch).load_state_dict(sd_c), N.NeRF(**arch).load_state_dict(sd_f)
    q = N.make_network_query_fn(N.get_embedder(10, 0)[0], N.get_embedder(4, 0)[0])
    H = W = a.hw
    origins, dirs, targets = [], [], []
    for theta in a.train_poses:
        K, c2w, near, far = synthetic.lego_camera(H, W, theta=theta)
        kw = dict(chunk=32768, c2w=c2w, ndc=False, near=near, far=far, use_viewdirs=True, network_fn=net_c, network_fine=net_f,
                  network_query_fn=q, N_samples=64, N_importance=128, white_bkgd=True, perturb=0., raw_noise_std=0.)
        rays = N.Camera.from_nerf_pose(c2w, H, W, float(K[0][0])).gen_rays()
        origins.append(rays.origins)
        dirs.append(rays.dirs)
        targets.append(N.render(H, W, K, **kw)[0].reshape(-1, 3).contiguous())
    origins, dirs, targets = torch.cat(origins), torch.cat(dirs), torch.cat(targets)
    gen = torch.Generator(device="cpu").manual_seed(0)

    def batch():
        k = torch.randint(0, origins.shape[0], (a.batch,), generator=gen).cuda()
        return N.Rays(origins[k].contiguous(), dirs[k].contiguous()), targets[k].contiguous()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), r

    def backward_kernel(g, rays, tape, cot, gd, gs):
        b = _lib.GridRenderBackwardArgs()
        b.origins, b.dirs, b.n_rays = rays.origins.data_ptr(), rays.dirs.data_ptr(), rays.origins.shape[0]
        b.grad_rgb, b.tape, b.grad_density, b.grad_sh, b.mask = cot.data_ptr(), tape.data_ptr(), gd.data_ptr(), gs.data_ptr(), 0
        b.use_skip, b.stream = 1, g.ctx.stream().value
        _lib.check(g.ctx.lib.nerf_grid_render_backward(g._handle(), C.byref(g.opt._to_c()), C.byref(b)))

    grids, trainers, modules = {}, {}, {}
    for R in a.reso:
        grids[R] = N.SparseGrid.from_nerf(net_f, -a.box, a.box, R, n_dirs=a.n_dirs)
        grids[R].accelerate()
        trainers[R] = N.GridTrainer(grids[R])
        modules[R] = N.GridModule(grids[R])
    legs = ("render", "forward_backward", "ag_forward", "ag_backward", "ag_kernel", "ag_step", "sample_forward", "sample_backward")
    t = {R: {leg: [] for leg in legs} for R in a.reso}
    pts = ((torch.rand((a.points, 3), generator=gen) * 2.0 - 1.0) * a.box).cuda()
    for step in range(a.warmup + a.steps):
        rays, gt = batch()
        for R in a.reso:
            g, tr, m = grids[R], trainers[R], modules[R]
            ms = {}
            ms["render"], ref = timed(lambda: g.volume_render(rays))
            tr.zero_grad()
            ms["forward_backward"], rgb = timed(lambda: tr.forward_backward(rays, gt))
            assert torch.equal(rgb, ref)
            m.zero_grad(set_to_none=True)
            ms["ag_forward"], out = timed(lambda: m.volume_render(rays))
            assert torch.equal(out, ref)
            loss = ((out - gt) ** 2).mean()
            tape = out.grad_fn.saved_tensors[4]      # (before the backward frees it)
            ms["ag_backward"], _ = timed(loss.backward)
            cot = ((out.detach() - gt) * (2.0 / out.numel())).contiguous()
            tr.zero_grad()
            ms["ag_kernel"], _ = timed(lambda: backward_kernel(g, rays, tape, cot, tr.grad_density, tr.grad_sh))
            assert float((tr.grad_sh - m.sh_data.grad).abs().max()) <= 1e-4 * float(m.sh_data.grad.abs().max())
            m.zero_grad(set_to_none=True)
            ms["ag_step"], _ = timed(lambda: ((m.volume_render(rays) - gt) ** 2).mean().backward())
            m.zero_grad(set_to_none=True)
            ms["sample_forward"], (dens, sh) = timed(lambda: m.sample(pts))
            ms["sample_backward"], _ = timed((dens.sum() + (sh * 0.5).sum()).backward)
            m.zero_grad(set_to_none=True)
            if step >= a.warmup:
                for leg in legs:
                    t[R][leg].append(ms[leg])
    out = {"metric": "grid_autograd", "setup": f"synthetic_pair(0) fine network baked over [-{a.box}, {a.box}], basis_dim 9, n_dirs "
           f"{a.n_dirs}, accelerated; batches of {a.batch} random rays of {len(a.train_poses)} lego poses at {H}x{W}, MSE against "
           f"render(); {a.points} sample points", "steps": a.steps, "warmup": a.warmup, "grids": {}}
    for R in a.reso:
        g = grids[R]
        med = {leg: float(np.median(t[R][leg])) for leg in legs}
        out["grids"][str(R)] = {
            "kept_nodes": g.capacity, "gradient_table_bytes": g.capacity * 4 * (1 + g.sh_data.shape[1]),
            "ms": med, "ms_min": {leg: float(np.min(t[R][leg])) for leg in legs}, "ms_max": {leg: float(np.max(t[R][leg])) for leg in legs},
            "ms_all": t[R],
            "zero_fill_and_accumulate_ms": med["ag_backward"] - med["ag_kernel"],
            "ag_step_over_forward_backward": med["ag_step"] / med["forward_backward"],
            "ag_kernels_over_forward_backward": (med["ag_forward"] + med["ag_kernel"]) / med["forward_backward"],
            "ag_rays_per_s": a.batch * 1e3 / med["ag_step"],
            "sample_points_per_s": a.points * 1e3 / med["sample_forward"],
            "sample_backward_points_per_s": a.points * 1e3 / med["sample_backward"],
        }
    line = json.dumps(out)
    print(line)
    if a.write:
        with open(os.path.join(ROOT, "profiles", "bench_grid_autograd.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
