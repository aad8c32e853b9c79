#!/usr/bin/env python3
"""Benchmark of the full Plenoxels objective under autograd (GridModule.tv / tv_color / sparsity_loss) on one MI355X.

    python bench_grid_objective.py [--steps 20] [--warmup 5] [--reso 128 256] [--batch 5000] [--write]

The bakes of bench_grid_train.py (synthetic_pair(0) fine network, SparseGrid.from_nerf over [-1.5, 1.5], basis_dim 9,
accelerate()) and its batches: --batch random pixels of the lego camera at --train-poses azimuths, targets from the network's
render(). Legs, alternated step by step in one process and timed with HIP events on the current stream after warm-up:
  trainer_step     GridTrainer.train_step with the four weights (fused backward with the beta and sparsity terms, both TV
                   gradients over 1 % of the nodes, RMSProp at learning rate 0)
  autograd_step    the same objective through GridModule: volume_render with log_transmit, MSE, l_tv * tv(cells),
                   l_tv_sh * tv_color(cells=cells) over 1 % random cells, l_s * sparsity_loss(rays).sum(), the beta term
                   written from log_transmit; loss.backward(); torch.optim.Adam at learning rate 0
  tv / tv_color / tv_color_1pct / sparsity_loss, each _fwd and _bwd: the new calls alone, dense over every cell except
                   tv_color_1pct (gradients set to None outside the timed region)
These are reported, not barred: there is no earlier path to these values to compare against.
Prints one JSON line and writes it to profiles/bench_grid_objective.json with --write.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
WEIGHTS = dict(lambda_tv=1e-5, lambda_tv_sh=1e-3, lambda_beta=1e-5, lambda_sparsity=1e-11)      # svox2's syn configuration


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--reso", type=int, nargs="+", default=[128, 256])
    p.add_argument("--batch", type=int, default=5000)
    p.add_argument("--n-dirs", type=int, default=64)
    p.add_argument("--box", type=float, default=1.5)
    p.add_argument("--hw", type=int, default=400)
    p.add_argument("--train-poses", type=float, nargs="+", default=[60.0 * i for i in range(6)])
    p.add_argument("--write", action="store_true")
    a = p.parse_args()
    torch.cuda.set_device(0)
    import nerf_projects_amd as N
    from nerf_projects_amd import synthetic
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
    dgen = torch.Generator(device="cuda").manual_seed(0)

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

    grids, trainers, modules, adams = {}, {}, {}, {}
    for R in a.reso:
        b = N.SparseGrid.from_nerf(net_f, -a.box, a.box, R, n_dirs=a.n_dirs)
        g = N.SparseGrid.from_tensors(b.links, b.density_data.clone(), b.sh_data.clone(), b.radius, b.center)
        g.opt = b.opt
        g.accelerate()
        grids[R], trainers[R], modules[R] = g, N.GridTrainer(g, generator=torch.Generator(device="cpu").manual_seed(1)), N.GridModule(g)
        adams[R] = torch.optim.Adam(modules[R].parameters(), lr=0.0)
    alone = ("tv", "tv_color", "tv_color_1pct", "sparsity_loss")
    legs = ("trainer_step", "autograd_step") + tuple(f"{n}_{d}" for n in alone for d in ("fwd", "bwd"))
    t = {R: {leg: [] for leg in legs} for R in a.reso}
    w = WEIGHTS
    for step in range(a.warmup + a.steps):
        rays, gt = batch()
        for R in a.reso:
            g, tr, m, adam = grids[R], trainers[R], modules[R], adams[R]
            nodes = g.links.numel()
            ms = {}
            ms["trainer_step"], _ = timed(lambda: tr.train_step(rays, gt, lr_sigma=0.0, lr_sh=0.0, tv_sh_ignore_edge=True, **w))

            def autograd_step():
                adam.zero_grad(set_to_none=True)
                cells = torch.randint(0, nodes, (max(1, nodes // 100),), device="cuda", generator=dgen)
                rgb, log_t = m.volume_render(rays, return_log_transmit=True)
                beta = (log_t + torch.log(1.0 - torch.exp(log_t) + 1e-3)).mean()
                loss = (((rgb - gt) ** 2).mean() + w["lambda_tv"] * m.tv(cells=cells) + w["lambda_tv_sh"] * m.tv_color(cells=cells)
                        + w["lambda_sparsity"] * m.sparsity_loss(rays).sum() + w["lambda_beta"] * beta)
                loss.backward()
                adam.step()
                return float(loss)      # (the read-back train_step pays too)

            ms["autograd_step"], _ = timed(autograd_step)
            cells = torch.randint(0, nodes, (max(1, nodes // 100),), device="cuda", generator=dgen)
            calls = {"tv": m.tv, "tv_color": m.tv_color, "tv_color_1pct": lambda: m.tv_color(cells=cells),
                     "sparsity_loss": lambda: m.sparsity_loss(rays).sum()}
            for name in alone:
                adam.zero_grad(set_to_none=True)
                ms[name + "_fwd"], v = timed(calls[name])
                ms[name + "_bwd"], _ = timed(v.backward)
            adam.zero_grad(set_to_none=True)
            if step >= a.warmup:
                for leg in legs:
                    t[R][leg].append(ms[leg])
    out = {"metric": "grid_objective", "setup": f"synthetic_pair(0) fine network baked over [-{a.box}, {a.box}], basis_dim 9, n_dirs "
           f"{a.n_dirs}, accelerated; batches of {a.batch} random rays of {len(a.train_poses)} lego poses at {H}x{W}; weights {WEIGHTS}",
           "steps": a.steps, "warmup": a.warmup, "grids": {}}
    for R in a.reso:
        med = {leg: float(np.median(t[R][leg])) for leg in legs}
        out["grids"][str(R)] = {"kept_nodes": grids[R].capacity, "cells": int(np.prod([s - 1 for s in grids[R].links.shape])),
                                "ms": med, "ms_min": {leg: float(np.min(t[R][leg])) for leg in legs},
                                "autograd_over_trainer": med["autograd_step"] / med["trainer_step"]}
    line = json.dumps(out)
    print(line)
    if a.write:
        with open(os.path.join(ROOT, "profiles", "bench_grid_objective.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
