#!/usr/bin/env python3
"""Benchmark of sparse voxel grid training (nerf-projects_amd/grid_train.py) on one MI355X.

    python bench_grid_train.py [--steps 20] [--warmup 5] [--reso 128 256] [--batch 5000] [--finetune-steps 500] [--lr-sigma 0.1]

The network of bench.py (synthetic_pair(0), 8 x 256, view directions) baked with SparseGrid.from_nerf(fine, -1.5, 1.5, R),
basis_dim 9, accelerate(). Training rays: batches of --batch random pixels (svox2's default batch_size) of the lego camera
at --train-poses azimuths (24 by default; theta = 30 is bench.py's), the targets are the network's own render() of those poses. Legs,
alternated step by step in one process and timed with HIP events on the current stream after warm-up:
  render           grid.volume_render(batch): the renderer the trainer's forward has to reproduce, the yardstick
  forward_backward trainer.forward_backward(batch, targets) (gradients zeroed outside the timed region)
  tv               trainer.add_tv_grad("density") + trainer.add_tv_grad("sh") over 1 % of the nodes each
  step             trainer.step(...) with the mask of the preceding forward_backward
  train_step       all of it, including zero_grad and the loss read-back
The timed legs run at learning rate 0 on a copy of the bake, so every step sees the same grid. Per R: steps/s and rays/s,
shaded samples per ray (instrumented launch of its own), the scattered bytes shaded x 8 x (4 + 12 B) B per second against the
1.3 TB/s the chip sustains in float atomics, and forward_backward / render.
Then the R = --finetune-reso bake is trained for --finetune-steps steps (lr_sh 1e-2, --lr-sigma) and the PSNR against the
network on a held-out pose is reported before and after (this measures the representation, not the kernels).
Prints one JSON line and writes it to profiles/bench_grid_train.json with --write.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
ATOMIC_TBPS = 1.3


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
    p.add_argument("--heldout-pose", type=float, default=37.5)
    p.add_argument("--finetune-reso", type=int, default=128)
    p.add_argument("--finetune-steps", type=int, default=500)
    p.add_argument("--lr-sigma", type=float, default=0.1)
    p.add_argument("--lr-sh", type=float, default=1e-2)
    p.add_argument("--lambda-tv", type=float, default=0.0)
    p.add_argument("--lambda-tv-sh", type=float, default=0.0)
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

    def pose(theta):
        K, c2w, near, far = synthetic.lego_camera(H, W, theta=theta)
        kw = dict(chunk=32768, c2w=c2w, ndc=False, near=near, far=far, use_viewdirs=True, network_fn=net_c, network_fine=net_f,
                  network_query_fn=q, N_samples=64, N_importance=128, white_bkgd=True, perturb=0., raw_noise_std=0.)
        cam = N.Camera.from_nerf_pose(c2w, H, W, float(K[0][0]))
        return cam, N.render(H, W, K, **kw)[0].reshape(-1, 3).contiguous()

    origins, dirs, targets = [], [], []
    for theta in a.train_poses:
        cam, rgb = pose(theta)
        rays = cam.gen_rays()
        origins.append(rays.origins)
        dirs.append(rays.dirs)
        targets.append(rgb)
    origins, dirs, targets = torch.cat(origins), torch.cat(dirs), torch.cat(targets)
    held_cam, held_rgb = pose(a.heldout_pose)
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

    def psnr(x, y):
        return float(-10.0 * np.log10(max(float(((x - y).double() ** 2).mean()), 1e-30)))

    grids, trainers, bakes = {}, {}, {}
    for R in a.reso:
        bakes[R] = N.SparseGrid.from_nerf(net_f, -a.box, a.box, R, n_dirs=a.n_dirs)
        b = bakes[R]
        grids[R] = N.SparseGrid.from_tensors(b.links, b.density_data.clone(), b.sh_data.clone(), b.radius, b.center)
        grids[R].opt = b.opt
        grids[R].accelerate()
        trainers[R] = N.GridTrainer(grids[R], generator=torch.Generator(device="cpu").manual_seed(1))
    legs = ("render", "forward_backward", "tv", "step", "train_step")
    t = {R: {leg: [] for leg in legs} for R in a.reso}
    shaded = {R: [] for R in a.reso}
    for step in range(a.warmup + a.steps):
        keep = step >= a.warmup
        rays, gt = batch()
        for R in a.reso:
            g, tr = grids[R], trainers[R]
            ms = {}
            ms["render"], ref = timed(lambda: g.volume_render(rays))
            tr.zero_grad()
            ms["forward_backward"], rgb = timed(lambda: tr.forward_backward(rays, gt))
            assert torch.equal(rgb, ref)
            ms["tv"], _ = timed(lambda: (tr.add_tv_grad("density", 1e-5), tr.add_tv_grad("sh", 1e-3)))
            ms["step"], _ = timed(lambda: tr.step(0.0, 0.0))
            ms["train_step"], _ = timed(lambda: tr.train_step(rays, gt, lr_sigma=0.0, lr_sh=0.0, lambda_tv=1e-5, lambda_tv_sh=1e-3))
            if keep:
                for leg in legs:
                    t[R][leg].append(ms[leg])
                shaded[R].append(g.count_samples(rays=rays)[1] / a.batch)
    out = {"metric": "grid_train", "setup": f"synthetic_pair(0) fine network baked over [-{a.box}, {a.box}], basis_dim 9, n_dirs {a.n_dirs}, "
           f"accelerated; batches of {a.batch} random rays of {len(a.train_poses)} lego poses at {H}x{W}, targets from render()",
           "steps": a.steps, "warmup": a.warmup, "atomic_rate_TBps": ATOMIC_TBPS, "grids": {}}
    for R in a.reso:
        g = grids[R]
        assert torch.equal(g.density_data, bakes[R].density_data) and torch.equal(g.sh_data, bakes[R].sh_data)      # lr 0
        med = {leg: float(np.median(t[R][leg])) for leg in legs}
        spr = float(np.mean(shaded[R]))
        scattered = spr * a.batch * 8 * (4 + 12 * 9)
        out["grids"][str(R)] = {
            "kept_nodes": g.capacity, "ms": med, "ms_all": t[R], "train_steps_per_s": 1e3 / med["train_step"],
            "train_rays_per_s": a.batch * 1e3 / med["train_step"], "forward_backward_rays_per_s": a.batch * 1e3 / med["forward_backward"],
            "shaded_per_ray": spr, "scattered_bytes_per_step": scattered,
            "scattered_TBps": scattered / (med["forward_backward"] * 1e-3) / 1e12,
            "scattered_fraction_of_atomic_rate": scattered / (med["forward_backward"] * 1e-3) / 1e12 / ATOMIC_TBPS,
            "forward_backward_over_render": med["forward_backward"] / med["render"],
        }
    # ---- fine-tune the bake against the network ----
    R = a.finetune_reso if a.finetune_reso in grids else a.reso[0]
    g, tr = grids[R], trainers[R]
    before = psnr(g.volume_render_image(held_cam).reshape(-1, 3), held_rgb)
    first = last = None
    for i in range(a.finetune_steps):
        rays, gt = batch()
        stats = tr.train_step(rays, gt, lr_sigma=a.lr_sigma, lr_sh=a.lr_sh, lambda_tv=a.lambda_tv, lambda_tv_sh=a.lambda_tv_sh)
        first = stats["psnr"] if first is None else first
        last = stats["psnr"]
    after = psnr(g.volume_render_image(held_cam).reshape(-1, 3), held_rgb)
    out["finetune"] = {"reso": R, "steps": a.finetune_steps, "lr_sigma": a.lr_sigma, "lr_sh": a.lr_sh, "lambda_tv": a.lambda_tv, "lambda_tv_sh": a.lambda_tv_sh, "beta": 0.95, "optim": "rmsprop",
                       "train_poses": len(a.train_poses),
                       "heldout_theta": a.heldout_pose, "heldout_psnr_before_db": before, "heldout_psnr_after_db": after,
                       "batch_psnr_first_db": first, "batch_psnr_last_db": last, "accelerated_after": bool(g.accelerated)}
    line = json.dumps(out)
    print(line)
    if a.write:
        with open(os.path.join(ROOT, "profiles", "bench_grid_train.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
