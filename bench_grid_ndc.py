#!/usr/bin/env python3
"""Benchmark of NDC cameras and NDC ray batches of the sparse voxel grid (NdcCamera, GridDataset with ndc_coeffs) on one
MI355X.

    python bench_grid_ndc.py [--steps 20] [--warmup 5] [--batch 5000] [--write]

Two legs, each an NDC call against its plain twin, alternated step by step in one process and timed with HIP events on the
current stream after warm-up; medians, and the spread (min and max) of each:

  frame   a 1008 x 756 frame (LLFF's size at scale 1/4) of a [256, 256, 128] bake of bench.py's network
          (SparseGrid.from_nerf of synthetic_pair(0) over [-1.5, 1.5]^3, basis_dim 9), plain and accelerated.
          `plain_camera`: the lego pose through a Camera, the grid in its own box. `ndc_camera`: the same tables in the box
          of a forward-facing scene (radius [1 + 500 / 1008, 1 + 500 / 756, 1] about 0) through an NdcCamera at the origin
          with LLFF fern's focal length. The two frames cross different parts of the grid, so beside the times stand the
          samples shaded per ray of each (an instrumented launch of its own): the ray set-up is a few dozen operations per
          ray against hundreds per shaded sample.
  batch   a --batch ray batch of the permuted order from a GridDataset of 20 images of 378 x 504 with and without
          ndc_coeffs: one launch each, both bound by the launch.
Prints one JSON line and writes it to profiles/bench_grid_ndc.json with --write.
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
    p.add_argument("--batch", type=int, default=5000)
    p.add_argument("--write", action="store_true")
    a = p.parse_args()
    torch.cuda.set_device(0)
    import nerf_projects_amd as N
    from nerf_projects_amd import synthetic

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), r

    def stats(v):
        return {"ms": float(np.median(v)), "ms_min_max": [float(np.min(v)), float(np.max(v))]}

    # ---- frame ----
    W, H, focal = 1008, 756, 815.0
    arch = dict(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=4, skips=[4], use_viewdirs=True)
    net_f = N.NeRF(**arch).load_state_dict(synthetic.synthetic_pair(0)[1])
    reso = [256, 256, 128]
    world = N.SparseGrid.from_nerf(net_f, -1.5, 1.5, reso)
    K, c2w, _, _ = synthetic.lego_camera(H, W)
    plain_cam = N.Camera.from_nerf_pose(c2w, H, W, float(K[0][0]))
    radius = [1 + 2 * 250 / W, 1 + 2 * 250 / H, 1.0]
    ndc = N.SparseGrid.from_tensors(world.links, world.density_data, world.sh_data, radius, [0.0, 0.0, 0.0])
    ndc.opt = world.opt
    ndc_cam = N.NdcCamera(torch.eye(4)[:3], focal, focal, W * 0.5, H * 0.5, width=W, height=H, ndc_coeffs=(2 * focal / W, 2 * focal / H))
    legs = {"plain_camera": (world, plain_cam), "ndc_camera": (ndc, ndc_cam)}
    frame = {}
    for mode in ("plain", "accelerated"):
        if mode == "accelerated":
            world.accelerate()
            ndc.accelerate()
        t = {k: [] for k in legs}
        for step in range(a.warmup + a.steps):
            for k, (g, cam) in legs.items():
                ms, _ = timed(lambda: g.volume_render_image(cam))
                if step >= a.warmup:
                    t[k].append(ms)
        frame[mode] = {k: stats(v) for k, v in t.items()}
        for k, (g, cam) in legs.items():
            visited, shaded = g.count_samples(camera=cam)
            frame[mode][k].update(visited_per_ray=visited / (W * H), shaded_per_ray=shaded / (W * H))
            frame[mode][k]["ns_per_shaded_sample"] = frame[mode][k]["ms"] * 1e6 / max(shaded, 1)
    img = ndc.volume_render_image(ndc_cam)
    assert torch.equal(img.view(-1, 3), ndc.volume_render(ndc_cam.gen_rays()))
    t_gen = {"plain_camera": [], "ndc_camera": []}
    for step in range(a.warmup + a.steps):
        for k, (_, cam) in legs.items():
            ms, _ = timed(cam.gen_rays)
            if step >= a.warmup:
                t_gen[k].append(ms)
    out = {"metric": "grid_ndc", "steps": a.steps, "warmup": a.warmup,
           "frame": {"setup": f"{W}x{H}, from_nerf of synthetic_pair(0) at {reso}, basis_dim 9, {world.capacity} rows", **frame,
                     "gen_rays": {k: stats(v) for k, v in t_gen.items()}}}

    # ---- batch ----
    rng = np.random.default_rng(0)
    n_img, h, w = 20, 378, 504
    images = rng.integers(0, 256, (n_img, h, w, 3), dtype=np.uint8)
    poses = np.tile(np.eye(4, dtype=np.float32)[None, :3], (n_img, 1, 1))
    poses[:, :, 3] = rng.uniform(-0.3, 0.3, (n_img, 3)).astype(np.float32)
    f = 407.5
    kw = dict(white_bkgd=False, generator=torch.Generator(device="cpu").manual_seed(0))
    sets = {"plain": N.GridDataset.from_arrays(images, poses, f, f, w / 2, h / 2, **kw),
            "ndc": N.GridDataset.from_arrays(images, poses, f, f, w / 2, h / 2, ndc_coeffs=(2 * f / w, 2 * f / h), **kw)}
    for ds in sets.values():
        ds.shuffle_rays()
    n_batches = sets["ndc"].n_rays // a.batch
    t = {k: [] for k in sets}
    for step in range(a.warmup + a.steps):
        b = (step % n_batches) * a.batch
        for k, ds in sets.items():
            ms, _ = timed(lambda: ds.batch(b, b + a.batch))
            if step >= a.warmup:
                t[k].append(ms)
    out["batch"] = {"setup": f"{n_img} images of {h}x{w}, permuted order, batches of {a.batch} rays", **{k: stats(v) for k, v in t.items()}}
    line = json.dumps(out)
    print(line)
    if a.write:
        with open(os.path.join(ROOT, "profiles", "bench_grid_ndc.json"), "w") as fobj:
            fobj.write(line + "\n")


if __name__ == "__main__":
    main()
