#!/usr/bin/env python3
"""Benchmark of sparse voxel grid resampling (nerf-projects_amd/grid_resample.py) on one MI355X.

    python bench_grid_resample.py [--steps 7] [--warmup 2] [--pairs 128:256 256:512] [--train-steps 200] [--write]

The network of bench.py (synthetic_pair(0), 8 x 256, view directions) baked with SparseGrid.from_nerf(fine, -1.5, 1.5, R),
basis_dim 9, as in bench_grid_train.py. For every pair R:R' the bake at R is resampled to R' (dilate 2). Legs, alternated
repetition by repetition in one process and timed with HIP events on the current stream after warm-up; medians with ranges:
  resample_sigma   resample_grid(grid, R', sigma_thresh=5, accelerate=False): the whole call, its one wait included
  composed_sigma   the same resample composed from what the package offered before this module: the lattice as a materialised
                   [N, 3] point tensor, grid.sample on it (in pieces of 2^24 points), torch for the threshold, the dilation
                   (max_pool3d), the cumulative-sum links, the index of kept points, grid.sample again for the colours -
                   svox2's own structure. The yardstick: resample_sigma must not be slower. The results are compared bit
                   for bit in the warm-up.
  resample_weight  resample_grid(grid, R', cameras=the 24 training poses, weight_thresh=0.01, accelerate=False)
  stages           lattice density, weight render (all cameras), threshold, dilate x 2, compact, gather, accelerate, each
                   between its own events, with the bytes the stage must move (every array it has to read or write, once;
                   for the weight render a lower bound: the volume read and the weights written once per call, although
                   24 cameras march through them) and the fraction of the chip's measured read rate (6.0 TB/s,
                   profiles/microbench/hbm_read_rate.hip) that is
  weight_render    one camera's weight render over the R' lattice density next to volume_render_image of that camera on the
                   resampled grid
Then quality, reported and not barred: PSNR against the network's own render of a held-out pose for the R = 128 bake, its
256 upsample (weight threshold, the training poses), that upsample after --train-steps training steps, and a direct R = 256
bake; with the kept-node counts. Prints one JSON line and writes it to profiles/bench_grid_resample.json with --write.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
READ_TBPS = 6.0
PIECE = 1 << 24


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=7)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--pairs", type=str, nargs="+", default=["128:256", "256:512"])
    p.add_argument("--n-dirs", type=int, default=64)
    p.add_argument("--box", type=float, default=1.5)
    p.add_argument("--hw", type=int, default=400)
    p.add_argument("--train-poses", type=float, nargs="+", default=[15.0 * i for i in range(24)])
    p.add_argument("--heldout-pose", type=float, default=37.5)
    p.add_argument("--train-steps", type=int, default=200)
    p.add_argument("--batch", type=int, default=5000)
    p.add_argument("--lr-sigma", type=float, default=0.1)
    p.add_argument("--lr-sh", type=float, default=1e-2)
    p.add_argument("--sigma-thresh", type=float, default=5.0)
    p.add_argument("--weight-thresh", type=float, default=0.01)
    p.add_argument("--write", action="store_true")
    a = p.parse_args()
    torch.cuda.set_device(0)
    import nerf_projects_amd as N
    from nerf_projects_amd import grid_resample as GR
    from nerf_projects_amd import synthetic
    arch = dict(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=4, skips=[4], use_viewdirs=True)
    sd_c, sd_f = synthetic.synthetic_pair(0)
    net_c, net_f = N.NeRF(**arch).load_state_dict(sd_c), N.NeRF(**arch).load_state_dict(sd_f)
    q = N.make_network_query_fn(N.get_embedder(10, 0)[0], N.get_embedder(4, 0)[0])
    H = W = a.hw

    def pose(theta, render=True):
        K, c2w, near, far = synthetic.lego_camera(H, W, theta=theta)
        cam = N.Camera.from_nerf_pose(c2w, H, W, float(K[0][0]))
        if not render:
            return cam, None
        kw = dict(chunk=32768, c2w=c2w, ndc=False, near=near, far=far, use_viewdirs=True, network_fn=net_c, network_fine=net_f,
                  network_query_fn=q, N_samples=64, N_importance=128, white_bkgd=True, perturb=0., raw_noise_std=0.)
        return cam, N.render(H, W, K, **kw)[0].reshape(-1, 3).contiguous()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), r

    def psnr(x, y):
        return float(-10.0 * np.log10(max(float(((x - y).double() ** 2).mean()), 1e-30)))

    def stat(v):
        return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}

    cams = [pose(t, render=False)[0] for t in a.train_poses]
    pairs = [tuple(int(x) for x in s.split(":")) for s in a.pairs]
    bakes = {}
    for R in sorted({r for r, _ in pairs} | {128, 256}):
        bakes[R] = N.SparseGrid.from_nerf(net_f, -a.box, a.box, R, n_dirs=a.n_dirs)
        bakes[R].accelerate()

    def composed(grid, R2):
        """svox2's resample from grid.sample and torch ops"""
        dev = grid.links.device
        reso = [R2] * 3
        axes = [x.to(dev) for x in GR.lattice_axes(list(grid.links.shape), reso)]
        points = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).view(-1, 3)
        dens = torch.cat([grid.sample(points[i:i + PIECE], grid_coords=True, want_colors=False)[0]
                          for i in range(0, points.shape[0], PIECE)]).view(reso)
        mask = dens >= a.sigma_thresh
        for _ in range(2):
            mask = torch.nn.functional.max_pool3d(mask[None, None].to(torch.float16), 3, 1, 1)[0, 0] > 0
        flat = mask.view(-1)
        kept = points[flat]
        sh = torch.cat([grid.sample(kept[i:i + PIECE], grid_coords=True, want_colors=True)[1]
                        for i in range(0, kept.shape[0], PIECE)]) if kept.shape[0] else torch.empty((0, grid.sh_data.shape[1]), device=dev)
        links = torch.cumsum(flat.to(torch.int32), 0, dtype=torch.int32) - 1
        links[~flat] = -1
        return links.view(reso), dens.view(-1)[flat].view(-1, 1), sh

    def stages(grid, R2, use_cams):
        """every stage between its own events; returns ({stage: ms}, {stage: bytes}, kept)"""
        ctx = grid.ctx
        reso = [R2] * 3
        n = R2 ** 3
        cols = grid.sh_data.shape[1]
        n_old, cap_old = grid.links.numel(), grid.capacity
        ms, by = {}, {}
        axes = GR._axes_arg(GR.lattice_axes(list(grid.links.shape), reso), reso, ctx)
        ms["lattice_density"], vol = timed(lambda: GR.lattice_density(grid, axes))
        by["lattice_density"] = 4 * n + 4 * n_old + 4 * cap_old
        source, thresh = vol, a.sigma_thresh
        if use_cams:
            source = torch.zeros(reso, device=ctx.device)

            def all_cams():
                for c in cams:
                    GR.weight_render(vol, c, grid.radius, grid.center, 0.5, 0.2, out=source)
            ms["weight_render"], _ = timed(all_cams)
            by["weight_render"] = 8 * n      # a lower bound: the volume read once, the weights written once (the march re-reads)
            thresh = a.weight_thresh
        ms["threshold"], mask = timed(lambda: GR.threshold_mask(source, thresh))
        by["threshold"] = 5 * n
        ms["dilate_x2"], mask = timed(lambda: GR.dilate_mask(mask, 2))
        by["dilate_x2"] = 2 * 2 * n
        ms["compact"], (links, count) = timed(lambda: GR.compact_mask(mask))
        by["compact"] = 2 * n + 4 * n
        rows = int(count.item())
        ms["gather"], (dens, sh) = timed(lambda: GR._gather(grid, axes, links, vol, rows))
        by["gather"] = 4 * n + rows * (4 + 4 + 4 + 4 * cols) + 4 * n_old + 4 * cols * cap_old
        new = N.SparseGrid.from_tensors(links, dens, sh, grid.radius, grid.center)
        ms["accelerate"], _ = timed(new.accelerate)
        by["accelerate"] = 4 * n + n + 2 * n * 31      # links read, bytes written, then 31 growth passes over the bytes (§7c)
        return ms, by, rows

    out = {"metric": "grid_resample", "setup": f"synthetic_pair(0) fine network baked over [-{a.box}, {a.box}], basis_dim 9, n_dirs "
           f"{a.n_dirs}; dilate 2, sigma_thresh {a.sigma_thresh}, weight_thresh {a.weight_thresh} with {len(cams)} lego poses at {H}x{W}",
           "steps": a.steps, "warmup": a.warmup, "read_rate_TBps": READ_TBPS, "pairs": {}}
    for R, R2 in pairs:
        g = bakes[R]
        legs = {k: [] for k in ("resample_sigma", "composed_sigma", "resample_weight")}
        st = {"sigma": {}, "weight": {}}
        kept = {}
        for step in range(a.warmup + a.steps):
            keep = step >= a.warmup
            ms = {}
            ms["resample_sigma"], new = timed(lambda: N.resample_grid(g, R2, sigma_thresh=a.sigma_thresh, accelerate=False))
            ms["composed_sigma"], ref = timed(lambda: composed(g, R2))
            if step == 0:      # the two paths compute the same grid
                assert torch.equal(new.links, ref[0]) and torch.equal(new.density_data, ref[1]) and torch.equal(new.sh_data, ref[2])
            kept["sigma"] = new.capacity
            del ref
            ms["resample_weight"], neww = timed(lambda: N.resample_grid(g, R2, weight_thresh=a.weight_thresh, cameras=cams, accelerate=False))
            kept["weight"] = neww.capacity
            for mode in ("sigma", "weight"):
                s_ms, s_by, rows = stages(g, R2, mode == "weight")
                assert rows == kept[mode]
                if keep:
                    for k, v in s_ms.items():
                        st[mode].setdefault(k, {"ms": [], "bytes": s_by[k]})["ms"].append(v)
            if keep:
                for k in legs:
                    legs[k].append(ms[k])
            del new
        rec = {"source_kept_nodes": g.capacity, "kept_nodes": kept, "legs_ms": {k: stat(v) for k, v in legs.items()}, "legs_ms_all": legs,
               "resample_over_composed": float(np.median(legs["resample_sigma"]) / np.median(legs["composed_sigma"])), "stages": {}}
        for mode in st:
            rec["stages"][mode] = {}
            for k, v in st[mode].items():
                m = float(np.median(v["ms"]))
                rec["stages"][mode][k] = {"ms": stat(v["ms"]), "bytes": v["bytes"],
                                          "TBps": None if v["bytes"] is None else v["bytes"] / (m * 1e-3) / 1e12,
                                          "fraction_of_read_rate": None if v["bytes"] is None else v["bytes"] / (m * 1e-3) / 1e12 / READ_TBPS}
        # one camera: the weight render over the lattice density next to the renderer on the resampled grid
        axes = GR.lattice_axes([R] * 3, [R2] * 3)
        vol = GR.lattice_density(g, axes)
        neww.accelerate()
        wr, vr = [], []
        for step in range(a.warmup + a.steps):
            w = torch.zeros_like(vol)
            t_w, _ = timed(lambda: GR.weight_render(vol, cams[2], g.radius, g.center, out=w))
            t_v, _ = timed(lambda: neww.volume_render_image(cams[2]))
            if step >= a.warmup:
                wr.append(t_w)
                vr.append(t_v)
        rec["weight_render_one_camera_ms"] = stat(wr)
        rec["volume_render_image_same_camera_ms"] = stat(vr)
        out["pairs"][f"{R}:{R2}"] = rec
        del vol, neww
        torch.cuda.empty_cache()
    # ---- quality: coarse to fine against a direct bake ----
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
    g128 = bakes[128]
    up = N.resample_grid(g128, 256, weight_thresh=a.weight_thresh, cameras=cams)
    qual = {"heldout_theta": a.heldout_pose, "train_steps": a.train_steps, "lr_sigma": a.lr_sigma, "lr_sh": a.lr_sh, "batch": a.batch,
         "bake_128": {"kept_nodes": g128.capacity, "psnr_db": psnr(g128.volume_render_image(held_cam).reshape(-1, 3), held_rgb)},
         "upsampled_256": {"kept_nodes": up.capacity, "psnr_db": psnr(up.volume_render_image(held_cam).reshape(-1, 3), held_rgb)},
         "bake_256": {"kept_nodes": bakes[256].capacity,
                      "psnr_db": psnr(bakes[256].volume_render_image(held_cam).reshape(-1, 3), held_rgb)}}
    tr = N.GridTrainer(up)
    for _ in range(a.train_steps):
        k = torch.randint(0, origins.shape[0], (a.batch,), generator=gen).cuda()
        tr.train_step(N.Rays(origins[k].contiguous(), dirs[k].contiguous()), targets[k].contiguous(), lr_sigma=a.lr_sigma, lr_sh=a.lr_sh)
    qual["upsampled_256_trained"] = {"kept_nodes": up.capacity, "psnr_db": psnr(up.volume_render_image(held_cam).reshape(-1, 3), held_rgb)}
    out["quality"] = qual
    line = json.dumps(out)
    print(line)
    if a.write:
        with open(os.path.join(ROOT, "profiles", "bench_grid_resample.json"), "w") as f:
            f.write(line + "\n")
    for key, rec in out["pairs"].items():      # the yardstick
        assert rec["legs_ms"]["resample_sigma"]["median"] <= rec["legs_ms"]["composed_sigma"]["median"], (key, rec["legs_ms"])


if __name__ == "__main__":
    main()
