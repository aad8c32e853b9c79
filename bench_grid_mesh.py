#!/usr/bin/env python3
"""Benchmark of surface-mesh extraction from a sparse voxel grid (nerf-projects_amd/grid_mesh.py) on one MI355X.

    python bench_grid_mesh.py [--steps 7] [--warmup 2] [--resos 128 256] [--write]

The network of bench.py (synthetic_pair(0), 8 x 256, view directions) baked with SparseGrid.from_nerf(fine, -1.5, 1.5, R),
basis_dim 9, at R = 128 and 256, in one process. The isovalue is the median of the positive densities of the R = 128 bake.
Legs, alternated repetition by repetition and timed by the wall clock around work that ends in a device synchronise (the
extraction waits for its counts anyway); medians with ranges:
  geometry     extract_mesh(grid, iso, normals=False, colors=None, world=False): the two counting passes, the scan, the wait
               for the counts, the two emitting passes
  composed     the parent path: the volume densified with torch indexing, then marching_cubes_volume - the same passes on a
               second [X, Y, Z] fp32 volume that has to be written and read. The two paths return the same bytes (asserted)
  normals      mesh_attributes(grid, vertices, colors=None)
  dc, sh, view mesh_attributes with that colour mode (normals included)
  render       render_colors at the vertices: one volume_render ray per vertex, on top of a "dc" pass
and V, T and the peak extra device memory of geometry and of composed (torch's allocator, above what is resident before the
call; the marching scratch lives in the context's workspace, reported as workspace_bytes). Prints one JSON line and, with
--write, writes it to profiles/bench_grid_mesh.json.
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
    p.add_argument("--steps", type=int, default=7)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--resos", type=int, nargs="+", default=[128, 256])
    p.add_argument("--n-dirs", type=int, default=64)
    p.add_argument("--box", type=float, default=1.5)
    p.add_argument("--write", action="store_true")
    a = p.parse_args()
    torch.cuda.set_device(0)
    import nerf_projects_amd as N
    from nerf_projects_amd import grid_mesh as GM
    from nerf_projects_amd import synthetic
    arch = dict(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=4, skips=[4], use_viewdirs=True)
    _, sd_f = synthetic.synthetic_pair(0)
    net_f = N.NeRF(**arch).load_state_dict(sd_f)

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, r

    def peak_extra(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        r = fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, r

    def stat(v):
        return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}

    def composed(grid, iso):
        links = grid.links
        vol = torch.where(links >= 0, grid.density_data[links.clamp(min=0).long(), 0], torch.zeros((), device=links.device))
        return N.marching_cubes_volume(vol, iso)

    def measure(grid, iso):
        view = (0.0, 0.6, -0.8)
        legs = {k: [] for k in ("geometry", "composed", "normals", "dc", "sh", "view", "render")}
        mesh = None
        for step in range(a.warmup + a.steps):
            ms = {}
            ms["geometry"], mesh = wall(lambda: N.extract_mesh(grid, iso, normals=False, colors=None, world=False))
            ms["composed"], (v, t) = wall(lambda: composed(grid, iso))
            if step == 0:
                assert torch.equal(v, mesh.vertices) and torch.equal(t, mesh.triangles)
            del v, t
            pts = mesh.vertices
            ms["normals"], (normals, _) = wall(lambda: N.mesh_attributes(grid, pts, colors=None))
            ms["dc"], (_, dc) = wall(lambda: N.mesh_attributes(grid, pts, colors="dc"))
            ms["sh"], _ = wall(lambda: N.mesh_attributes(grid, pts, colors="sh"))
            ms["view"], _ = wall(lambda: N.mesh_attributes(grid, pts, view=view))
            ms["render"], _ = wall(lambda: GM.render_colors(grid, pts, normals, dc))
            if step >= a.warmup:
                for k in legs:
                    legs[k].append(ms[k])
        mem_geometry, _ = peak_extra(lambda: N.extract_mesh(grid, iso, normals=False, colors=None, world=False))
        mem_composed, _ = peak_extra(lambda: composed(grid, iso))
        n = grid.links.numel()
        V, T = int(mesh.vertices.shape[0]), int(mesh.triangles.shape[0])
        rec = {"nodes": n, "kept_nodes": grid.capacity, "V": V, "T": T, "legs_ms": {k: stat(v) for k, v in legs.items()},
               "legs_ms_all": legs, "output_bytes": 12 * V + 24 * T, "peak_extra_bytes": {"geometry": mem_geometry, "composed": mem_composed},
               "workspace_bytes": int(grid.ctx.lib.nerf_workspace_bytes(grid.ctx.handle)),
               "geometry_over_composed": float(np.median(legs["geometry"]) / np.median(legs["composed"]))}
        return rec

    out = {"metric": "grid_mesh", "setup": f"synthetic_pair(0) fine network baked over [-{a.box}, {a.box}], basis_dim 9, n_dirs "
           f"{a.n_dirs}; iso = the median positive density of the first bake", "steps": a.steps, "warmup": a.warmup, "grids": {}}
    iso = None
    for R in a.resos:
        grid = N.SparseGrid.from_nerf(net_f, -a.box, a.box, R, n_dirs=a.n_dirs)
        if iso is None:
            d = grid.density_data[:, 0]
            iso = float(d[d > 0].median())
            out["iso"] = iso
        out["grids"][f"{R}"] = measure(grid, iso)
        del grid
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.write:
        with open(os.path.join(ROOT, "profiles", "bench_grid_mesh.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
