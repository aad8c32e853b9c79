#!/usr/bin/env python3
"""Benchmark of training the sparse voxel grid's background layers (BackgroundTrainer) on one MI355X.

    python bench_grid_background_train.py [--steps 20] [--warmup 3] [--reso 128 256] [--batch 5000] [--nlayers 64] [--bg-reso 512]

The scene of bench_grid_background.py: the network of bench.py baked with SparseGrid.from_nerf(fine, -1.5, 1.5, R),
basis_dim 9, accelerated, and the synthetic background of `nlayers` layers of 2 bg-reso x bg-reso texels; batches of `batch`
random rays of the 800 x 800 lego camera (a new batch every step) towards the render of the untrained scene plus noise. Legs,
alternated step by step in one process and timed with HIP events on the current stream after warm-up, medians in ms:
  foreground R   GridTrainer(grid.foreground()).train_step      the step without layers (tables of its own)
  full R         BackgroundTrainer(grid).train_step             the comparison of record: full - foreground = the background's share
  taped R        nerf_grid_background_rays_taped alone          on the batch's taped foreground
  backward R     nerf_grid_background_backward alone            on the same batch; backward / taped is recorded
The library named by NERF_MI355X_LIB is the one measured (an ablation build of nerf-projects_amd/build.py, for the A/B of the
backward's mapping). Prints one JSON line.
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
from bench_grid_background import synthetic_background  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reso", type=int, nargs="+", default=[128, 256])
    p.add_argument("--n-dirs", type=int, default=64)
    p.add_argument("--box", type=float, default=1.5)
    p.add_argument("--hw", type=int, default=800)
    p.add_argument("--batch", type=int, default=5000)
    p.add_argument("--nlayers", type=int, default=64)
    p.add_argument("--bg-reso", type=int, default=512)
    a = p.parse_args()
    if a.steps < 1 or a.warmup < 0 or a.batch < 1:
        p.error("--steps >= 1, --warmup >= 0 and --batch >= 1 are required")
    torch.cuda.set_device(0)
    import nerf_projects_amd as N
    from nerf_projects_amd import _lib, synthetic
    from nerf_projects_amd._lib import GridBackgroundBackwardArgs, GridBackgroundTapedArgs, GridRenderTapedArgs, check
    arch = dict(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=4, skips=[4], use_viewdirs=True)
    _, sd_f = synthetic.synthetic_pair(0)
    net_f = N.NeRF(**arch).load_state_dict(sd_f)
    H = W = a.hw
    K, c2w, _, _ = synthetic.lego_camera(H, W)
    cam = N.Camera.from_nerf_pose(c2w, H, W, float(K[0][0]))
    bg_links, bg_data = synthetic_background(a.nlayers, a.bg_reso, "cuda")
    rays_all = cam.gen_rays()
    gen = torch.Generator(device="cpu").manual_seed(0)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), r

    scenes = {}
    for R in a.reso:
        baked = N.SparseGrid.from_nerf(net_f, -a.box, a.box, R, n_dirs=a.n_dirs)
        g = N.BackgroundGrid.from_tensors(baked.links, baked.density_data.clone(), baked.sh_data.clone(), baked.radius, baked.center,
                                          basis_dim=baked.basis_dim, background_links=bg_links, background_data=bg_data.clone())
        g.opt = baked.opt
        g.accelerate()
        target = g.volume_render(rays_all)
        target = (target + 0.05 * torch.randn(target.shape, generator=gen).to(target.device)).clamp(0.0, 1.0)
        baked.accelerate()
        scenes[R] = dict(full=N.BackgroundTrainer(g), fg=N.GridTrainer(baked), target=target)

    def alone(R, idx):
        """the two background calls on the batch's taped foreground, each timed alone"""
        tr = scenes[R]["full"]
        g, ctx = tr.grid, tr.ctx
        h, lib, stream = g._handle(), ctx.lib, ctx.stream().value
        o, d = rays_all.origins[idx].contiguous(), rays_all.dirs[idx].contiguous()
        n = o.shape[0]
        opt, fg_opt = g.opt._to_c(False), g.opt._to_c(False)
        fg_opt.background_brightness = 0.0
        rgb = torch.empty((n, 3), device=o.device)
        logt_fg, logt = torch.empty((n,), device=o.device), torch.empty((n,), device=o.device)
        tape = torch.empty((n, 3), device=o.device, dtype=torch.float64)
        tape_bg = torch.empty_like(tape)
        t = GridRenderTapedArgs()
        t.origins, t.dirs, t.n_rays, t.rgb_out, t.log_transmit, t.tape = o.data_ptr(), d.data_ptr(), n, rgb.data_ptr(), logt_fg.data_ptr(), tape.data_ptr()
        t.use_skip, t.stream = 1, stream
        check(lib.nerf_grid_render_rays_taped(h, C.byref(fg_opt), C.byref(t)))
        b = GridBackgroundTapedArgs()
        b.origins, b.dirs, b.n_rays, b.rgb = o.data_ptr(), d.data_ptr(), n, rgb.data_ptr()
        b.log_transmit, b.log_transmit_out, b.tape, b.tape_background = logt_fg.data_ptr(), logt.data_ptr(), tape.data_ptr(), tape_bg.data_ptr()
        b.stream = stream
        ms_taped, _ = timed(lambda: check(lib.nerf_grid_background_rays_taped(h, C.byref(opt), C.byref(b))))
        grad_rgb = ((rgb - scenes[R]["target"][idx]) * (2.0 / (3.0 * n))).contiguous()
        tr.grad_background.zero_()
        tr.mask_background.zero_()
        w = GridBackgroundBackwardArgs()
        w.origins, w.dirs, w.n_rays, w.grad_rgb = o.data_ptr(), d.data_ptr(), n, grad_rgb.data_ptr()
        w.log_transmit, w.tape_background = logt_fg.data_ptr(), tape_bg.data_ptr()
        w.grad_background, w.mask_background, w.stream = tr.grad_background.data_ptr(), tr.mask_background.data_ptr(), stream
        ms_bwd, _ = timed(lambda: check(lib.nerf_grid_background_backward(h, C.byref(opt), C.byref(w))))
        return ms_taped, ms_bwd, float((logt_fg < -25).float().mean()), int(tr.mask_background.sum())

    times = {R: {"foreground": [], "full": [], "taped": [], "backward": []} for R in a.reso}
    info = {R: {} for R in a.reso}
    lr = dict(lr_sigma=1.0, lr_sh=1e-3)
    for step in range(a.warmup + a.steps):
        idx = torch.randint(0, H * W, (a.batch,), generator=gen).cuda()
        rays = N.Rays(rays_all.origins[idx].contiguous(), rays_all.dirs[idx].contiguous())
        for R in a.reso:
            s = scenes[R]
            gt = s["target"][idx].contiguous()
            ms_fg, _ = timed(lambda: s["fg"].train_step(rays, gt, **lr))
            ms_full, out = timed(lambda: s["full"].train_step(rays, gt, lr_sigma_bg=0.1, lr_color_bg=1e-3, **lr))
            ms_taped, ms_bwd, dark, touched = alone(R, idx)
            if step >= a.warmup:
                for leg, ms in (("foreground", ms_fg), ("full", ms_full), ("taped", ms_taped), ("backward", ms_bwd)):
                    times[R][leg].append(ms)
            info[R] = dict(rays_left_alone=dark, mask_entries_touched=touched, mse=out["mse"])

    def stats(v):
        return {"ms": float(np.median(v)), "ms_min": float(np.min(v)), "ms_all": v}
    out = {"metric": "grid_background_train_step", "scene": f"synthetic_pair(0) fine network baked over [-{a.box}, {a.box}], basis_dim 9, "
           f"n_dirs {a.n_dirs}, step_size 0.5, accelerated; background {a.nlayers} layers of {2 * a.bg_reso} x {a.bg_reso}; batches of "
           f"{a.batch} random rays of the lego {H}x{W} camera", "steps": a.steps, "warmup": a.warmup,
           "library": os.path.basename(_lib.library_path()), "background_bytes": bg_data.numel() * 4, "grids": {}}
    for R in a.reso:
        res = {leg: stats(v) for leg, v in times[R].items()}
        res["kept_nodes"] = scenes[R]["full"].grid.capacity
        res["full_minus_foreground_ms"] = res["full"]["ms"] - res["foreground"]["ms"]
        res["backward_over_taped"] = res["backward"]["ms"] / res["taped"]["ms"]
        res.update(info[R])
        assert np.isfinite(res["mse"])
        out["grids"][str(R)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
