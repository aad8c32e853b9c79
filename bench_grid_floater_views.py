#!/usr/bin/env python3
"""Benchmark of the floater views of a sparse voxel grid (nerf-projects_amd/grid_floater_views.py) on one MI355X.

    python bench_grid_floater_views.py [--steps 10] [--warmup 3] [--resos 128 256] [--hw 800] [--specks 50000] [--write]

The network of bench.py (synthetic_pair(0), 8 x 256, view directions) baked with SparseGrid.from_nerf(fine, -1.5, 1.5, R),
basis_dim 9, at R = 128 and 256, as in bench_grid_components.py, with its seeded sprinkling of about --specks single kept
nodes (density 10) over the empty space, so that there are floaters to draw; accelerate(); the 800 x 800 lego camera.
compute_FDR is timed once by the wall clock. Then, alternated repetition by repetition in one process and timed with HIP
events on the current stream after warm-up, per view; medians with ranges:
  depth         volume_render_depth_image(camera, sigma_thresh=0.0): the threshold depth frame, the yardstick
  colour        volume_render_image(camera)
  heatmap       project_floaters_to_view(..., depth_map=that depth): the scan, the counts and the dilation
  heatmap+depth project_floaters_to_view(...) with its own depth frame
  view          component_view(..., min_viz_size=0): the table (with its wait for the volumes when min_viz_size > 0 - not here),
                the scan with up to 21 atomicMin per drawn node, the resolve
with each as a ratio to the depth frame. No pass/fail bar. Prints one JSON line and writes it to
profiles/bench_grid_floater_views.json with --write.
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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--resos", type=int, nargs="+", default=[128, 256])
    p.add_argument("--hw", type=int, default=800)
    p.add_argument("--specks", type=int, default=50000)
    p.add_argument("--n-dirs", type=int, default=64)
    p.add_argument("--box", type=float, default=1.5)
    p.add_argument("--write", action="store_true")
    a = p.parse_args()
    torch.cuda.set_device(0)
    import nerf_projects_amd as N
    from nerf_projects_amd import synthetic
    arch = dict(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=4, skips=[4], use_viewdirs=True)
    _, sd_f = synthetic.synthetic_pair(0)
    net_f = N.NeRF(**arch).load_state_dict(sd_f)
    H = W = a.hw
    K, c2w, _, _ = synthetic.lego_camera(H, W)
    cam = N.Camera.from_nerf_pose(c2w, H, W, float(K[0][0]))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), r

    def stat(v):
        return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}

    def speckled(grid, seed):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        n = grid.links.numel()
        dust = (grid.links < 0) & (torch.rand(grid.links.shape, device="cuda", generator=gen) < a.specks / n)
        extra = int(dust.sum())
        links = grid.links.clone()
        links[dust] = grid.capacity + torch.arange(extra, dtype=torch.int32, device="cuda")
        dens = torch.cat([grid.density_data, torch.full((extra, 1), 10.0, device="cuda")])
        sh = torch.cat([grid.sh_data, torch.zeros((extra, grid.sh_data.shape[1]), device="cuda")])
        return N.SparseGrid.from_tensors(links, dens, sh, grid.radius, grid.center)

    out = {"metric": "grid_floater_views", "setup": f"synthetic_pair(0) fine network baked over [-{a.box}, {a.box}], basis_dim 9, "
           f"n_dirs {a.n_dirs}, about {a.specks} single nodes of density 10 in empty space, accelerated; {H} x {W} lego camera",
           "steps": a.steps, "warmup": a.warmup, "grids": {}}
    for R in a.resos:
        grid = speckled(N.SparseGrid.from_nerf(net_f, -a.box, a.box, R, n_dirs=a.n_dirs), R)
        grid.accelerate()
        torch.cuda.synchronize()
        t = time.perf_counter()
        fdr = N.compute_FDR(grid)
        torch.cuda.synchronize()
        fdr_ms = (time.perf_counter() - t) * 1e3
        legs = {k: [] for k in ("depth", "colour", "heatmap", "heatmap+depth", "view")}
        counts = None
        for step in range(a.warmup + a.steps):
            ms = {}
            ms["depth"], depth = timed(lambda: grid.volume_render_depth_image(cam, sigma_thresh=0.0))
            ms["colour"], _ = timed(lambda: grid.volume_render_image(cam))
            ms["heatmap"], heat = timed(lambda: N.project_floaters_to_view(grid, fdr, cam, depth_map=depth))
            ms["heatmap+depth"], _ = timed(lambda: N.project_floaters_to_view(grid, fdr, cam))
            ms["view"], slots = timed(lambda: N.component_view(grid, fdr, cam, min_viz_size=0))
            if step == 0:
                _, counts = N.project_floaters_to_view(grid, fdr, cam, depth_map=depth, return_counts=True)
            if step >= a.warmup:
                for k in legs:
                    legs[k].append(ms[k])
        d = float(np.median(legs["depth"]))
        out["grids"][f"{R}+specks"] = {
            "nodes": grid.links.numel(), "kept_nodes": grid.capacity, "num_components": fdr["num_components"],
            "num_floaters": fdr["num_floaters"], "floater_volume": fdr["floater_volume"], "main_volume": fdr["main_volume"],
            "counters": counts, "heatmap_max": float(heat.max()), "pixels_drawn": int((slots > 0).sum()),
            "compute_FDR_ms": fdr_ms, "legs_ms": {k: stat(v) for k, v in legs.items()}, "legs_ms_all": legs,
            "over_depth_frame": {k: float(np.median(v)) / d for k, v in legs.items()}}
        del grid, fdr
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.write:
        with open(os.path.join(ROOT, "profiles", "bench_grid_floater_views.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
