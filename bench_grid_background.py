#!/usr/bin/env python3
"""Benchmark of the sparse voxel grid's background layers (BackgroundGrid) on one MI355X.

    python bench_grid_background.py [--steps 20] [--warmup 3] [--reso 128 256] [--hw 800] [--nlayers 64] [--bg-reso 512]

The scene of bench_grid.py: the network of bench.py (synthetic_pair(0), 8 x 256, view directions) baked with
SparseGrid.from_nerf(fine, -1.5, 1.5, R), basis_dim 9, after accelerate(), the 800 x 800 lego camera, and a synthetic
background of `nlayers` layers of 2 bg-reso x bg-reso texels: smooth random sigma (a sum of low-frequency waves over the
sphere and the layers, about half of it positive, up to 4) and smooth random colours. Legs, alternated step by step in one
process and timed with HIP events on the current stream after warm-up:
  foreground R   grid.foreground().volume_render_image(camera)     the frame without layers
  full R         grid.volume_render_image(camera)                  foreground, then the background pass: the comparison of record
  pass           the frame of a grid without a kept node: the background pass alone (every ray crosses every layer), as an
                 image and through the rays form with the camera's rays in row order
  sparsify       grid.sparsify_background(1.0, 1) on a fresh copy of the background (with its one host read)
Per R also: the share of rays the pass leaves alone (foreground log_transmit < -25), and that the frame equals the render of
the camera's rays bit for bit. The library named by NERF_MI355X_LIB is the one measured (an ablation build of
nerf-projects_amd/build.py, for the A/B of the pixel mapping). Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def synthetic_background(nlayers, reso, device, seed=0):
    """links [2 R, R] (every texel has a row) and data [2 R^2, L, 4], smooth in all three directions"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    lon = torch.linspace(-np.pi, np.pi, 2 * reso + 1, device=device)[:-1].view(-1, 1, 1)
    lat = torch.linspace(np.pi / 2, -np.pi / 2, reso, device=device).view(1, -1, 1)
    lay = torch.linspace(0.0, 1.0, nlayers, device=device).view(1, 1, -1)
    data = torch.zeros((2 * reso, reso, nlayers, 4), device=device)
    for c in range(4):
        for _ in range(6):
            k = torch.randint(1, 5, (3,), generator=gen).tolist()
            ph = (torch.rand(3, generator=gen) * 2 * np.pi).tolist()
            data[..., c] += torch.sin(k[0] * lon + ph[0]) * torch.cos(k[1] * lat + ph[1]) * torch.sin(np.pi * k[2] * lay + ph[2])
    data[..., 3] = (data[..., 3] * 1.5).clamp(max=4.0)
    links = torch.arange(2 * reso * reso, dtype=torch.int32, device=device).view(2 * reso, reso)
    return links, data.view(2 * reso * reso, nlayers, 4).contiguous()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reso", type=int, nargs="+", default=[128, 256])
    p.add_argument("--n-dirs", type=int, default=64)
    p.add_argument("--box", type=float, default=1.5)
    p.add_argument("--hw", type=int, default=800)
    p.add_argument("--nlayers", type=int, default=64)
    p.add_argument("--bg-reso", type=int, default=512)
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
    bg_links, bg_data = synthetic_background(a.nlayers, a.bg_reso, "cuda")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), r

    grids, fgs = {}, {}
    for R in a.reso:
        fg = N.SparseGrid.from_nerf(net_f, -a.box, a.box, R, n_dirs=a.n_dirs)
        fg.accelerate()
        g = N.BackgroundGrid.from_tensors(fg.links, fg.density_data, fg.sh_data, fg.radius, fg.center, basis_dim=fg.basis_dim,
                                          background_links=bg_links, background_data=bg_data)
        g.opt = fg.opt
        g.accelerate()
        grids[R], fgs[R] = g, fg
    # the pass alone: a foreground without a kept node, so that every ray arrives with log_transmit 0
    empty = N.BackgroundGrid(reso=8, radius=a.box, basis_dim=9, background_nlayers=a.nlayers, background_reso=a.bg_reso)
    empty.links[:] = -1
    empty.background_links, empty.background_data = bg_links, bg_data
    empty.opt = grids[a.reso[0]].opt
    rays = cam.gen_rays()

    def sparsify():
        s = N.BackgroundGrid.from_tensors(empty.links, empty.density_data, empty.sh_data, empty.radius, empty.center, basis_dim=9,
                                          background_links=bg_links.clone(), background_data=bg_data)
        return timed(lambda: s.sparsify_background(1.0, 1))

    times = {R: {"foreground": [], "full": []} for R in a.reso}
    times["pass"], times["pass_image"], times["sparsify"] = [], [], []
    kept = None
    for step in range(a.warmup + a.steps):
        for R in a.reso:
            for leg, fn in (("foreground", lambda: fgs[R].volume_render_image(cam)), ("full", lambda: grids[R].volume_render_image(cam))):
                ms, _ = timed(fn)
                if step >= a.warmup:
                    times[R][leg].append(ms)
        ms_rays, _ = timed(lambda: empty.volume_render(rays))
        ms_img, _ = timed(lambda: empty.volume_render_image(cam))
        ms_sp, kept = sparsify()
        if step >= a.warmup:
            times["pass"].append(ms_rays)
            times["pass_image"].append(ms_img)
            times["sparsify"].append(ms_sp)

    def stats(v):
        return {"ms": float(np.median(v)), "ms_min": float(np.min(v)), "ms_all": v}
    out = {"metric": "grid_background_frame", "frame": f"lego {H}x{W}, synthetic_pair(0) fine network baked over [-{a.box}, {a.box}], "
           f"basis_dim 9, n_dirs {a.n_dirs}, step_size 0.5, accelerated; background {a.nlayers} layers of {2 * a.bg_reso} x {a.bg_reso}",
           "steps": a.steps, "warmup": a.warmup, "library": os.path.basename(_lib.library_path()),
           "background_bytes": bg_data.numel() * 4, "pass_rays": stats(times["pass"]), "pass_image_on_empty_foreground": stats(times["pass_image"]),
           "sparsify": dict(stats(times["sparsify"]), kept_rows=kept, rows=int(bg_data.shape[0])), "grids": {}}
    for R in a.reso:
        g, fg = grids[R], fgs[R]
        assert g.accelerated and fg.accelerated
        res = {"kept_nodes": g.capacity, "foreground": stats(times[R]["foreground"]), "full": stats(times[R]["full"])}
        res["full_over_foreground"] = res["full"]["ms"] / res["foreground"]["ms"]
        res["full_minus_foreground_ms"] = res["full"]["ms"] - res["foreground"]["ms"]
        img = g.volume_render_image(cam)
        rgb, logt = g.volume_render(rays, return_log_transmit=True)
        assert torch.equal(img.view(-1, 3), rgb) and torch.isfinite(img).all()
        fg_logt = fg.volume_render(rays, return_log_transmit=True)[1]
        res["rays_left_alone"] = float((fg_logt < -25).float().mean())
        res["pixels"] = H * W
        out["grids"][str(R)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
