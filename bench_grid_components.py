#!/usr/bin/env python3
"""Benchmark of floater detection on a sparse voxel grid (nerf-projects_amd/grid_components.py) on one MI355X.

    python bench_grid_components.py [--steps 7] [--warmup 2] [--resos 128 256 512] [--specks 50000] [--write]

The network of bench.py (synthetic_pair(0), 8 x 256, view directions) baked with SparseGrid.from_nerf(fine, -1.5, 1.5, R),
basis_dim 9, at R = 128 and 256, and the 256 bake resampled to 512 (sigma_thresh 5, dilate 2), as in bench_grid_resample.py.
Every grid is measured as it is and again with a seeded sprinkling of about --specks single kept nodes (density 10) over its
empty space, so that the component count reaches 10^4 - 10^5. Legs, alternated repetition by repetition in one process and
timed with HIP events on the current stream after warm-up; medians with ranges:
  occupancy     links + one density per kept node -> a byte per node
  labelling     union-find (init, merge, flatten + root count, scan, rank, spread) and the one wait for the count
  volumes       the histogram of the labels
  accelerate    grid.accelerate() on the same grid: the yardstick. At R = 256 occupancy + labelling + volumes must not take
                longer (asserted at the end, after the results are printed and written)
  compute_FDR   the whole call by the wall clock, host classification included
  remove        remove_floaters(grid, accelerate=False) by the wall clock
  scipy         when scipy is importable (3 repetitions at most above 2^26 nodes): the reference's path on the same
                occupancy - the copy of links and densities to the host, the dense array, ndimage.label + ndimage.sum - by
                the wall clock, and its ratio to compute_FDR; else null
with the bytes every stage must move (every array it has to read or write, once) and the fraction of the chip's measured
read rate (6.0 TB/s, profiles/microbench/hbm_read_rate.hip) that is. Prints one JSON line and writes it to
profiles/bench_grid_components.json with --write.
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
READ_TBPS = 6.0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=7)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--resos", type=int, nargs="+", default=[128, 256, 512])
    p.add_argument("--specks", type=int, default=50000)
    p.add_argument("--n-dirs", type=int, default=64)
    p.add_argument("--box", type=float, default=1.5)
    p.add_argument("--threshold", type=float, default=0.01)
    p.add_argument("--connectivity", type=int, default=26)
    p.add_argument("--write", action="store_true")
    a = p.parse_args()
    torch.cuda.set_device(0)
    import nerf_projects_amd as N
    from nerf_projects_amd import grid_components as GC
    from nerf_projects_amd import synthetic
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    arch = dict(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=4, skips=[4], use_viewdirs=True)
    _, sd_f = synthetic.synthetic_pair(0)
    net_f = N.NeRF(**arch).load_state_dict(sd_f)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), r

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, r

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

    def scipy_path(grid):
        """What the reference does with the same grid: host copies, a dense array, label, sum."""
        links = grid.links.cpu()
        active = links >= 0
        dense = torch.zeros(links.shape, dtype=torch.float32)
        dense[active] = grid.density_data[links[active].long().cuda(), 0].cpu()
        occ = (dense.numpy() > a.threshold).astype(np.uint8)
        labeled, n = ndimage.label(occ, structure=np.ones((3, 3, 3), dtype=np.uint8) if a.connectivity == 26 else None)
        vol = np.array(ndimage.sum(occ, labeled, range(1, n + 1)))
        return labeled, vol

    def measure(grid):
        n, cap = grid.links.numel(), grid.capacity
        legs = {k: [] for k in ("occupancy", "labelling", "volumes", "accelerate", "compute_FDR", "remove")}
        if ndimage is not None and a.connectivity in (6, 26):
            legs["scipy"] = []
        res = count = None
        scipy_reps = a.steps if n <= 1 << 26 else min(a.steps, 3)      # (seconds per repetition at 512^3)
        for step in range(a.warmup + a.steps):
            ms = {}
            ms["occupancy"], occ = timed(lambda: GC.occupancy(grid, a.threshold, True))
            ms["labelling"], (labels, count) = timed(lambda: GC.label_mask(occ, a.connectivity))
            ms["volumes"], vol = timed(lambda: GC.component_volumes(labels, count))
            ms["accelerate"], _ = timed(grid.accelerate)
            ms["compute_FDR"], res = wall(lambda: N.compute_FDR(grid, threshold=a.threshold, connectivity=a.connectivity))
            ms["remove"], (new, _) = wall(lambda: N.remove_floaters(grid, accelerate=False, threshold=a.threshold,
                                                                    connectivity=a.connectivity))
            if "scipy" in legs and (step == 0 or len(legs["scipy"]) < scipy_reps):
                ms["scipy"], (labeled, vol_ref) = wall(lambda: scipy_path(grid))
                if step == 0:      # the two paths label alike
                    assert np.array_equal(labeled, labels.cpu().numpy()) and np.array_equal(vol_ref, vol.cpu().numpy())
                del labeled
            del new
            if step >= a.warmup:
                for k in legs:
                    if k in ms:
                        legs[k].append(ms[k])
        by = {"occupancy": 4 * n + 4 * cap + n,
              # occupancy read by init, merge, flatten, rank, spread; parents written, read and rewritten by the occupied nodes;
              # labels written once per node
              "labelling": 5 * n + 4 * n + 3 * 4 * res["total_volume"],
              "volumes": 4 * n + 4 * count,
              "accelerate": 4 * n + n + 2 * n * 31}
        rec = {"nodes": n, "kept_nodes": cap, "num_components": count, "FDR": res["FDR"], "num_floaters": res["num_floaters"],
               "num_main_objects": res.get("num_main_objects", 0), "total_volume": res["total_volume"],
               "detection_method": res.get("detection_method", ""), "legs_ms": {k: stat(v) for k, v in legs.items()},
               "legs_ms_all": legs, "stages": {}}
        for k, b in by.items():
            m = float(np.median(legs[k]))
            rec["stages"][k] = {"bytes": b, "TBps": b / (m * 1e-3) / 1e12, "fraction_of_read_rate": b / (m * 1e-3) / 1e12 / READ_TBPS}
        device = sum(float(np.median(legs[k])) for k in ("occupancy", "labelling", "volumes"))
        rec["device_ms"] = device
        rec["device_over_accelerate"] = device / float(np.median(legs["accelerate"]))
        rec["scipy_over_compute_FDR"] = (float(np.median(legs["scipy"]) / np.median(legs["compute_FDR"])) if "scipy" in legs else None)
        return rec

    out = {"metric": "grid_components", "setup": f"synthetic_pair(0) fine network baked over [-{a.box}, {a.box}], basis_dim 9, n_dirs "
           f"{a.n_dirs}; 512 = the 256 bake resampled (sigma_thresh 5, dilate 2); threshold {a.threshold}, connectivity "
           f"{a.connectivity}; specks: about {a.specks} single nodes of density 10 in empty space",
           "steps": a.steps, "warmup": a.warmup, "read_rate_TBps": READ_TBPS, "scipy": ndimage is not None, "grids": {}}
    bake256 = None
    for R in a.resos:
        if R in (128, 256):
            grid = N.SparseGrid.from_nerf(net_f, -a.box, a.box, R, n_dirs=a.n_dirs)
            if R == 256:
                bake256 = grid
        else:
            if bake256 is None:
                bake256 = N.SparseGrid.from_nerf(net_f, -a.box, a.box, 256, n_dirs=a.n_dirs)
            grid = N.resample_grid(bake256, R, sigma_thresh=5.0, dilate=2, accelerate=False)
        out["grids"][f"{R}"] = measure(grid)
        dusty = speckled(grid, R)
        out["grids"][f"{R}+specks"] = measure(dusty)
        del dusty
        if R != 256:
            del grid
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.write:
        with open(os.path.join(ROOT, "profiles", "bench_grid_components.json"), "w") as f:
            f.write(line + "\n")
    for key in ("256", "256+specks"):      # the condition
        if key in out["grids"]:
            assert out["grids"][key]["device_over_accelerate"] <= 1.0, (key, out["grids"][key]["legs_ms"])


if __name__ == "__main__":
    main()
