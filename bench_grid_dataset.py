#!/usr/bin/env python3
"""Benchmark of the sparse voxel grid's training data and training driver (nerf-projects_amd/grid_dataset.py, grid_fit.py)
on one MI355X.

    python bench_grid_dataset.py [--steps 500] [--warmup 20] [--repeats 5] [--batch 5000] [--reso 128] [--hw 400] [--write]

The camera set of bench_grid_train.py (the lego camera at --train-poses azimuths, 24 by default, --hw x --hw) with synthetic
RGBA images (a shaded disc over a transparent background, different per pose). Three measurements in one process:

  batch     a --batch ray batch of an epoch in the permuted order from GridDataset.batch (one launch), against the
            reference's design on the same device: a pre-generated [N, 9] fp32 table (origin, direction, colour of every
            ray), shuffled once per epoch by indexing it with a device randperm (`shuffle`, also given per batch of the
            epoch), and a batch that is a slice of the shuffled table made contiguous (`table_batch`). HIP events on the
            current stream, medians after warm-up. Bytes resident in both designs (the table design holds two tables while
            it shuffles).
  driver    train_grid for --steps steps (opt.py's defaults: both TV terms on, RMSProp, print_every 20; one resolution, so
            no resample falls into the timed steps; timed from the first shuffle_rays, after the grid is made, to the end)
            against a bare loop of the same trainer calls on batches made beforehand. Wall clock around a device
            synchronisation, --repeats runs of each, alternated; the steps per second of every run, the medians, and the
            spread (min and max) of both.
Prints one JSON line and writes it to profiles/bench_grid_dataset.json with --write.
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


def synthetic_images(n, hw):
    """uint8 [n, hw, hw, 4]: a shaded disc whose colour and place depend on the pose, alpha 0 outside."""
    y, x = np.mgrid[0:hw, 0:hw].astype(np.float32) / hw
    out = np.zeros((n, hw, hw, 4), dtype=np.uint8)
    for i in range(n):
        a = 2 * np.pi * i / n
        cx, cy = 0.5 + 0.1 * np.cos(a), 0.5 + 0.1 * np.sin(a)
        r2 = (x - cx) ** 2 + (y - cy) ** 2
        inside = r2 < 0.09
        shade = np.clip(1.0 - r2 / 0.09, 0, 1)
        rgb = np.asarray([0.5 + 0.5 * np.cos(a), 0.5 + 0.5 * np.sin(a), 0.6], dtype=np.float32) * shade[..., None]
        out[i, ..., :3] = (255 * rgb).astype(np.uint8) * inside[..., None]
        out[i, ..., 3] = 255 * inside
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=500)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--batch", type=int, default=5000)
    p.add_argument("--reso", type=int, default=128)
    p.add_argument("--hw", type=int, default=400)
    p.add_argument("--train-poses", type=float, nargs="+", default=[15.0 * i for i in range(24)])
    p.add_argument("--write", action="store_true")
    a = p.parse_args()
    torch.cuda.set_device(0)
    import nerf_projects_amd as N
    from nerf_projects_amd import synthetic
    from nerf_projects_amd.grid_fit import GridTrainConfig, expon_lr, train_grid

    H = W = a.hw
    poses, focal = [], None
    for theta in a.train_poses:
        K, c2w, _, _ = synthetic.lego_camera(H, W, theta=theta)
        cam = N.Camera.from_nerf_pose(c2w, H, W, float(K[0][0]))
        poses.append(cam.c2w.numpy())
        focal = float(K[0][0])
    poses = np.stack(poses)
    poses[:, :3, 3] *= 2 / 3      # the scene inside the unit box, as svox2's scene_scale
    images = synthetic_images(len(poses), a.hw)
    ds = N.GridDataset.from_arrays(images, poses, focal, focal, W * 0.5 + 0.5, H * 0.5 + 0.5,
                                   generator=torch.Generator(device="cpu").manual_seed(0))
    n_rays = ds.n_rays
    batches_per_epoch = (n_rays - 1) // a.batch + 1

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), r

    # ---- batch: the kernel against the table design ----
    chunk = 1 << 20
    table = torch.cat([torch.cat([r.origins, r.dirs, gt], 1) for r, gt in
                       (ds.batch(b, min(b + chunk, n_rays)) for b in range(0, n_rays, chunk))])      # index order: not shuffled yet
    assert tuple(table.shape) == (n_rays, 9)
    ds.shuffle_rays()
    t = {"kernel_batch": [], "table_batch": [], "shuffle": []}
    shuffled = table
    for i in range(a.warmup + a.steps):
        b = (i % (batches_per_epoch - 1)) * a.batch
        ms_k, _ = timed(lambda: ds.batch(b, b + a.batch))
        ms_t, _ = timed(lambda: (shuffled[b:b + a.batch, 0:3].contiguous(), shuffled[b:b + a.batch, 3:6].contiguous(),
                                 shuffled[b:b + a.batch, 6:9].contiguous()))
        if i >= a.warmup:
            t["kernel_batch"].append(ms_k)
            t["table_batch"].append(ms_t)
    for i in range(3 + 7):
        ms_s, shuffled = timed(lambda: table[torch.randperm(n_rays, device=table.device)])
        if i >= 3:
            t["shuffle"].append(ms_s)
    med = {k: float(np.median(v)) for k, v in t.items()}
    out = {"metric": "grid_dataset",
           "setup": f"{len(poses)} lego poses at {H}x{W}, synthetic RGBA images, factor 1, batches of {a.batch} rays, permuted order",
           "rays": n_rays, "batches_per_epoch": batches_per_epoch, "steps": a.steps, "warmup": a.warmup,
           "batch": {"ms": med, "kernel_rays_per_s": a.batch * 1e3 / med["kernel_batch"],
                     "shuffle_ms_per_batch_of_the_epoch": med["shuffle"] / batches_per_epoch,
                     "table_design_ms_per_batch": med["table_batch"] + med["shuffle"] / batches_per_epoch,
                     "ms_min_max": {k: [float(np.min(v)), float(np.max(v))] for k, v in t.items()}},
           "bytes_resident": {"images_and_poses": ds.bytes_resident, "table": table.numel() * 4,
                              "table_while_shuffling": 2 * table.numel() * 4 + 8 * n_rays}}
    del table, shuffled
    torch.cuda.empty_cache()

    # ---- driver: train_grid against a bare loop of the same calls ----
    cfg = GridTrainConfig(reso=[[a.reso] * 3], n_iters=a.steps, batch_size=a.batch)
    lrs = [(expon_lr(s, cfg.lr_sigma, cfg.lr_sigma_final, cfg.lr_sigma_delay_steps, cfg.lr_sigma_delay_mult, cfg.lr_sigma_decay_steps),
            expon_lr(s, cfg.lr_sh, cfg.lr_sh_final, cfg.lr_sh_delay_steps, cfg.lr_sh_delay_mult, cfg.lr_sh_decay_steps))
           for s in range(a.steps)]
    clock = {}

    class Timed(N.GridDataset):      # the driver's clock starts at its first shuffle_rays: the grid has been made by then
        def shuffle_rays(self):
            if "t0" not in clock:
                torch.cuda.synchronize()
                clock["t0"] = time.perf_counter()
            return super().shuffle_rays()

    def make_grid():
        g = N.SparseGrid(reso=[a.reso] * 3, use_sphere_bound=True, basis_dim=cfg.sh_dim, use_z_order=True)
        g.density_data.fill_(cfg.init_sigma)
        g.opt.sigma_thresh, g.opt.stop_thresh = cfg.sigma_thresh, cfg.stop_thresh
        return g

    def run_driver(seed):
        d = Timed.from_arrays(ds.images_u8, ds.c2w, focal, focal, W * 0.5 + 0.5, H * 0.5 + 0.5,
                              generator=torch.Generator(device="cpu").manual_seed(seed))
        clock.clear()
        train_grid(d, cfg, generator=torch.Generator(device="cpu").manual_seed(seed))
        torch.cuda.synchronize()
        return a.steps / (time.perf_counter() - clock["t0"])

    def run_bare(seed):
        ds.generator.manual_seed(seed)
        ds.shuffle_rays()
        made = [ds.batch(s * a.batch, (s + 1) * a.batch) for s in range(a.steps)]
        tr = N.GridTrainer(make_grid(), generator=torch.Generator(device="cpu").manual_seed(seed))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for (rays, gt), (lr_sigma, lr_sh) in zip(made, lrs):
            tr.zero_grad()
            tr.forward_backward(rays, gt)
            tr.add_tv_grad("density", cfg.lambda_tv, cfg.tv_sparsity)
            tr.add_tv_grad("sh", cfg.lambda_tv_sh, cfg.tv_sh_sparsity, ignore_edge=True)
            tr.step(lr_sigma, lr_sh, beta=cfg.rms_beta, optim=cfg.sigma_optim)
        torch.cuda.synchronize()
        return a.steps / (time.perf_counter() - t0)

    assert a.steps <= batches_per_epoch
    run_bare(100), run_driver(100)      # warm-up of both
    bare, driver = [], []
    for r in range(a.repeats):
        bare.append(run_bare(r))
        driver.append(run_driver(r))
    out["driver"] = {"reso": a.reso, "steps_per_run": a.steps, "repeats": a.repeats,
                     "bare_steps_per_s": bare, "driver_steps_per_s": driver,
                     "bare_median": float(np.median(bare)), "driver_median": float(np.median(driver)),
                     "bare_spread": [float(np.min(bare)), float(np.max(bare))],
                     "driver_spread": [float(np.min(driver)), float(np.max(driver))],
                     "driver_median_not_below_bare_spread": bool(np.median(driver) >= np.min(bare))}
    line = json.dumps(out)
    print(line)
    if a.write:
        with open(os.path.join(ROOT, "profiles", "bench_grid_dataset.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
