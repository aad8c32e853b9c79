"""Writes tests/golden/grid_depth.npz: what ties the sparse voxel grid's depth and ray-length calls to the reference's svox2.

    NERF_REFERENCE_SVOX2=/path/to/reference/svox2 python tests/golden/make_golden_grid_depth.py

The reference computes depth only in CUDA. Two things of it run on the CPU (pure PyTorch) and are recorded here; nothing of
the reference is copied, the fixture holds arrays only.

1. Ray lengths: ``SparseGrid._volume_render_gradcheck_lerp(rays, return_raylen=True)`` on the grids a - d and the rays of
   tests/golden/grid_render.npz, in fp32 and in fp64, at ``near_clip`` 0 and for grid a also at 6.0. ``raylen_d_ref`` = the
   largest |fp32 - fp64| over the finite rays.
2. Expected depth out of the reference's RENDERER, by position-coded colours. Grid "e" is dense with ``basis_dim`` 1, its
   outermost node layer has density exactly 0, and the SH DC coefficient of node (i, j, k) is ((i / X, j / Y, k / Z) - 0.5) / C0:
   the colour of a sample is its grid position divided by the size (trilinear interpolation of an affine function is exact,
   colours lie in [0, 1) so the clamp never acts; a sample whose position is clamped interpolates the empty outer layer only
   and weighs nothing). With c0 / c1 the renders at background brightness 0 / 1:  T = c1 - c0;  sum w pos = c0 * size;
   sum w t = (c0 * size - (1 - T) o_grid) . d_grid  (d_grid unit, grid units);  depth = sum w t * delta_scale.
   ``e_depth64`` / ``e_T64`` come from the fp64 render; ``e_d_ref`` = the largest distance of the same derivation from the
   fp32 render: the reference's own distance from exact arithmetic. The PyTorch renderer has no ``sigma_thresh`` and no early
   stop: this is the semantics at ``sigma_thresh = 0``, ``stop_thresh = 0``.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_grid as MG  # noqa: E402  (imports the reference's svox2)

svox2 = MG.svox2
SH_C0 = 0.28209479177387814
E_RESO, E_RADIUS, E_CENTER = (12, 10, 14), (1.0, 0.8, 1.2), (0.1, -0.2, 0.3)


def reference(g, o, d, dt, near_clip=0.0, bg=1.0, raylen=False):
    g.opt.background_brightness, g.opt.step_size, g.opt.near_clip = bg, 0.5, near_clip
    torch.set_default_dtype(dt)
    try:
        with torch.no_grad():
            rays = svox2.Rays(torch.from_numpy(o).to(dt), torch.from_numpy(d).to(dt))
            return g._volume_render_gradcheck_lerp(rays, return_raylen=raylen).numpy()
    finally:
        torch.set_default_dtype(torch.float32)


def ray_lengths(out):
    z = np.load(os.path.join(HERE, "grid_render.npz"))
    d_ref = 0.0
    for name, reso, radius, center, basis_dim in MG.GRIDS:
        o, d = z[f"{name}_origins"], z[f"{name}_dirs"]
        grids = [MG.ref_grid(reso, radius, center, basis_dim, z[f"{name}_links"], z[f"{name}_density"], z[f"{name}_sh"], dt)
                 for dt in (torch.float32, torch.float64)]
        for tag, near in (("", 0.0), ("_near", 6.0)) if name == "a" else (("", 0.0),):
            r32 = reference(grids[0], o, d, torch.float32, near, raylen=True)
            r64 = reference(grids[1], o, d, torch.float64, near, raylen=True)
            assert r32.dtype == np.float32 and r64.dtype == np.float64 and r32.shape == (len(o),)
            fin = np.isfinite(r32) & np.isfinite(r64)
            dist = float(np.abs(r32[fin].astype(np.float64) - r64[fin]).max())
            d_ref = max(d_ref, dist)
            out[f"{name}_raylen{tag}"] = r32
            out[f"{name}_raylen{tag}64"] = r64
            print(f"grid {name} near_clip {near}: ray lengths in [{r32[fin].min():.3f}, {r32[fin].max():.3f}], {int((r32 < 0).sum())} "
                  f"misses, {int((~fin).sum())} not finite, |fp32 - fp64| max {dist:.3e}")
    out["raylen_near"] = np.float64(6.0)
    out["raylen_d_ref"] = np.float64(d_ref)


def grid_e(rng, out):
    X, Y, Z = E_RESO
    n = X * Y * Z
    links = np.arange(n, dtype=np.int32).reshape(E_RESO)
    density = (np.round(rng.uniform(-4.0, 20.0, E_RESO) * 16) / 16)
    density[[0, -1]] = density[:, [0, -1]] = density[:, :, [0, -1]] = 0.0
    i, j, k = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij")
    sh = ((np.stack([i / X, j / Y, k / Z], -1) - 0.5) / SH_C0).reshape(n, 3)
    density, sh = density.reshape(n, 1).astype(np.float32), sh.astype(np.float32)
    o, d = MG.make_rays(rng, E_RADIUS, E_CENTER)
    size = np.array(E_RESO, dtype=np.float64)
    # the set-up in fp64 from the fp32 radius and center, as the reference's fp64 grid has it
    radius, center = np.array(E_RADIUS, np.float32).astype(np.float64), np.array(E_CENTER, np.float32).astype(np.float64)
    o_grid = (0.5 * (1.0 - center / radius) * size - 0.5) + o.astype(np.float64) * (0.5 / radius * size)
    v = d.astype(np.float64) / np.linalg.norm(d.astype(np.float64), axis=-1, keepdims=True)
    d_grid = v * (0.5 / radius * size)
    delta_scale = 1.0 / np.linalg.norm(d_grid, axis=-1)
    d_grid *= delta_scale[:, None]
    res = {}
    for dt in (torch.float32, torch.float64):
        g = MG.ref_grid(E_RESO, E_RADIUS, E_CENTER, 1, links, density, sh, dt)
        c0 = reference(g, o, d, dt, bg=0.0).astype(np.float64)
        c1 = reference(g, o, d, dt, bg=1.0).astype(np.float64)
        assert c0.min() >= 0.0 and c0.max() < 1.0
        T = (c1 - c0).mean(-1)
        wt = ((c0 * size - (1.0 - T)[:, None] * o_grid) * d_grid).sum(-1)
        res[dt] = (wt * delta_scale, T)
    depth64, T64 = res[torch.float64]
    d_ref = float(np.abs(res[torch.float32][0] - depth64).max())
    hit = depth64 > 1e-9
    print(f"grid e: {int(hit.sum())} of {len(o)} rays with depth > 0, depth up to {depth64.max():.3f}, T down to {T64.min():.3e}, "
          f"|fp32 - fp64| max {d_ref:.3e}")
    assert hit.mean() >= 0.8 and depth64.min() > -1e-12
    out.update({"e_links": links, "e_density": density, "e_sh": sh, "e_origins": o, "e_dirs": d,
                "e_radius": np.array(E_RADIUS, np.float32), "e_center": np.array(E_CENTER, np.float32),
                "e_depth64": depth64, "e_T64": T64, "e_d_ref": np.float64(d_ref)})


def main():
    out = {}
    ray_lengths(out)
    grid_e(np.random.default_rng(20240915), out)
    path = os.path.join(HERE, "grid_depth.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
