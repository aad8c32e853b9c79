#!/usr/bin/env python3
"""Benchmark of the beta / sparsity losses and the edge-aware colour TV of sparse voxel grid training on one MI355X.

    python bench_grid_train_losses.py [--steps 20] [--warmup 5] [--reso 128 256] [--batch 5000] [--lambda-beta 1e-5] [--lambda-sparsity 1e-11]

The set-up of bench_grid_train.py: the network of bench.py (synthetic_pair(0), 8 x 256, view directions) baked with
SparseGrid.from_nerf(fine, -1.5, 1.5, R), basis_dim 9, accelerate(); batches of --batch random pixels of the lego camera at
--train-poses azimuths, the targets the network's own render(). Legs, alternated step by step in one process and timed with HIP
events on the current stream after warm-up, the gradients zeroed outside the timed region:
  forward_backward   trainer.forward_backward(batch, targets): the kernel without the terms
  fused_off          trainer.volume_render_fused(batch, targets): both weights 0, which launches that same kernel
  fused_on           trainer.volume_render_fused(batch, targets, beta_loss, sparsity_loss): the kernel with the terms
  tv_sh              trainer.add_tv_grad("sh") over 1 % of the nodes
  tv_sh_edge         trainer.add_tv_grad("sh", ignore_edge=True) over the same nodes
Per R: the median, the smallest and the largest of each leg, fused_on / fused_off and tv_sh_edge / tv_sh, and the run-to-run
spread (largest - smallest) / median of the off legs, against which the ratios are to be read.
Prints one JSON line and writes it to profiles/bench_grid_train_losses.json with --write.
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
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--reso", type=int, nargs="+", default=[128, 256])
    p.add_argument("--batch", type=int, default=5000)
    p.add_argument("--n-dirs", type=int, default=64)
    p.add_argument("--box", type=float, default=1.5)
    p.add_argument("--hw", type=int, default=400)
    p.add_argument("--train-poses", type=float, nargs="+", default=[45.0 * i for i in range(8)])
    p.add_argument("--lambda-beta", type=float, default=1e-5)
    p.add_argument("--lambda-sparsity", type=float, default=1e-11)
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

    grids, trainers = {}, {}
    for R in a.reso:
        grids[R] = N.SparseGrid.from_nerf(net_f, -a.box, a.box, R, n_dirs=a.n_dirs)
        grids[R].accelerate()
        trainers[R] = N.GridTrainer(grids[R])
    legs = ("forward_backward", "fused_off", "fused_on", "tv_sh", "tv_sh_edge")
    t = {R: {leg: [] for leg in legs} for R in a.reso}
    for step in range(a.warmup + a.steps):
        rays, gt = batch()
        for R in a.reso:
            g, tr = grids[R], trainers[R]
            start = int(torch.randint(0, g.links.numel(), (1,), generator=gen).item())
            ms = {}
            tr.zero_grad()
            ms["forward_backward"], ref = timed(lambda: tr.forward_backward(rays, gt))
            tr.zero_grad()
            ms["fused_off"], rgb = timed(lambda: tr.volume_render_fused(rays, gt))
            assert torch.equal(rgb, ref)
            tr.zero_grad()
            ms["fused_on"], rgb = timed(lambda: tr.volume_render_fused(rays, gt, beta_loss=a.lambda_beta, sparsity_loss=a.lambda_sparsity))
            assert torch.equal(rgb, ref)
            tr.zero_grad()
            ms["tv_sh"], _ = timed(lambda: tr.add_tv_grad("sh", 1e-3, start=start))
            tr.zero_grad()
            ms["tv_sh_edge"], _ = timed(lambda: tr.add_tv_grad("sh", 1e-3, start=start, ignore_edge=True))
            if step >= a.warmup:
                for leg in legs:
                    t[R][leg].append(ms[leg])
    out = {"metric": "grid_train_losses", "setup": f"synthetic_pair(0) fine network baked over [-{a.box}, {a.box}], basis_dim 9, n_dirs "
           f"{a.n_dirs}, accelerated; batches of {a.batch} random rays of {len(a.train_poses)} lego poses at {H}x{W}; lambda_beta "
           f"{a.lambda_beta}, lambda_sparsity {a.lambda_sparsity}", "steps": a.steps, "warmup": a.warmup, "grids": {}}
    for R in a.reso:
        med = {leg: float(np.median(t[R][leg])) for leg in legs}
        spread = {leg: (max(t[R][leg]) - min(t[R][leg])) / med[leg] for leg in legs}
        out["grids"][str(R)] = {
            "kept_nodes": grids[R].capacity, "ms": med, "ms_min": {leg: min(t[R][leg]) for leg in legs},
            "ms_max": {leg: max(t[R][leg]) for leg in legs}, "spread": spread,
            "fused_on_over_off": med["fused_on"] / med["fused_off"], "fused_off_over_forward_backward": med["fused_off"] / med["forward_backward"],
            "tv_sh_edge_over_tv_sh": med["tv_sh_edge"] / med["tv_sh"],
        }
    line = json.dumps(out)
    print(line)
    if a.write:
        with open(os.path.join(ROOT, "profiles", "bench_grid_train_losses.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
