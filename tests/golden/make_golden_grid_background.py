"""Writes tests/golden/grid_background.npz: a sparse voxel grid, backgrounds of 2, 5 and 8 layers, rays, and what the
reference's own classes compute for the geometry of the background pass.

    NERF_REFERENCE_SVOX2=/path/to/reference/svox2 python tests/golden/make_golden_grid_background.py

Runs on the CPU (``svox2`` imports without its CUDA extension). Nothing of the reference is copied: the fixture holds arrays
only. The background's specification is the reference's CUDA kernel (include/nerf_mi355x.h, "Sparse voxel grid: background
layers"), which cannot run here; its geometry is the formulas of ``utils.ConcentricSpheresIntersector`` and
``utils.xyz2equirect``, and those are recorded in fp32 and in fp64 (``ref32_*`` / ``ref64_*``): ``origins``, ``dirs``,
``world_step_scale``, the inner radius, ``intersect(r_i)`` for every radius of two settings and ``xyz2equirect`` of the
normalised hits. The inputs of those classes are the foreground set-up's fp32 ``o``, ``d``, ``delta_scale``
(tests/grid_oracle.py), which the fixture also holds, with the foreground's colour and log_transmit per setting.
``d_ref`` = the largest |oracle fp32 - oracle fp64| of what the pass returns (colour and log_transmit) over every ray,
background and setting, ``d_ref_rgb`` that of the colour alone (tests/grid_background_oracle.py: an independent
restatement, never the kernel).

Asserted on the inputs: no ray has |inner - r_i| < 1e-4 for any radius of any setting (that branch is discontinuous), no
ray stops in one precision and not in the other, and the coverage counts printed at the end.
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF = os.environ.get("NERF_REFERENCE_SVOX2")
if not REF:
    sys.exit("set NERF_REFERENCE_SVOX2 to the svox2 directory of the reference checkout (the one that holds svox2/svox2.py)")
sys.path.insert(0, REF)
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    import svox2  # noqa: E402  (reference)
    from svox2 import utils as ref_utils  # noqa: E402

import grid_background_oracle as BO  # noqa: E402
import grid_oracle as GO  # noqa: E402
from make_golden_grid import make_grid  # noqa: E402

F = np.float32
RESO, BASIS_DIM = (12, 14, 10), 4
RADIUS, CENTER = (1.5, 2.1, 1.8), (0.3, -0.2, 0.1)
BG_RESO, NLAYERS = 8, (2, 5, 8)
N_RAYS = 512
BRIGHTNESS = 0.7
# (nlayers, step_size, stop_thresh) of every recorded setting; the two marked settings also record intersect / equirect
SETTINGS = [(2, 0.5, 1e-7), (2, 0.3, 0.05), (5, 0.5, 1e-7), (5, 0.5, 0.05), (5, 0.3, 1e-7), (5, 0.3, 0.05), (8, 0.5, 1e-7),
            (8, 0.3, 0.05)]
GEOMETRY = [(5, 0.3), (2, 0.5)]      # 18 and 6 radii


def make_background(rng, nlayers):
    R = BG_RESO
    texels = 2 * R * R
    kept = rng.random(texels) >= 0.25
    n = int(kept.sum())
    links = np.full(texels, -1, dtype=np.int32)
    links[kept] = rng.permutation(n).astype(np.int32)
    data = np.empty((n, nlayers, 4), dtype=F)
    data[..., :3] = np.round(rng.normal(0.0, 2.0, (n, nlayers, 3)) * 64) / 64
    data[..., 3] = np.round(rng.uniform(-1.0, 6.0, (n, nlayers)) * 16) / 16
    return links.reshape(2 * R, R), data


def make_rays(rng):
    radius, center = np.array(RADIUS), np.array(CENTER)
    o = np.empty((N_RAYS, 3))
    d = np.empty((N_RAYS, 3))

    def unit(k):
        u = rng.normal(size=(k, 3))
        return u / np.linalg.norm(u, axis=-1, keepdims=True)
    # 0..351: inside the unit sphere of the normalised box, any direction, not unit
    k = np.arange(0, 352)
    o[k] = center + radius * unit(len(k)) * rng.uniform(0.0, 0.9, (len(k), 1))
    d[k] = unit(len(k)) * rng.uniform(0.3, 3.0, (len(k), 1))
    # 352..383: outside the sphere (some inside the box's corners, some beyond the box): inner > 1, negative t
    k = np.arange(352, 384)
    o[k] = center + radius * unit(len(k)) * rng.uniform(1.15, 2.5, (len(k), 1))
    d[k] = unit(len(k))
    # 384..399: exactly +-z and +-y (the seam and the poles), from beside the axis through the centre
    # (on that axis the longitude of a hit is the ratio of two rounding errors)
    k = np.arange(384, 400)
    axes = np.array([[0, 0, 1], [0, 0, -1], [0, 1, 0], [0, -1, 0]], dtype=np.float64)
    d[k] = np.tile(axes, (4, 1)) * np.repeat([1.0, 0.5, 2.0, 1.0], 4)[:, None]
    o[k] = center + radius * rng.uniform(0.1, 0.3, (len(k), 3)) * rng.choice([-1.0, 1.0], (len(k), 3))
    # 400..431: towards -z with a small sideways part of either sign: samples interpolated across the seam
    k = np.arange(400, 432)
    o[k] = center + radius * rng.uniform(-0.2, 0.2, (len(k), 3))
    d[k] = np.stack([rng.uniform(-0.08, 0.08, len(k)), rng.uniform(-0.8, 0.8, len(k)), -np.ones(len(k))], -1)
    # 432..479: outside the box, pointing away: miss the foreground, still cross every layer
    k = np.arange(432, 480)
    u = unit(len(k))
    o[k] = center + 3.0 * radius * u
    d[k] = u * radius + rng.normal(size=(len(k), 3)) * 0.1
    # 480..495: not finite
    k = np.arange(480, 496)
    o[k] = center + radius * rng.uniform(-0.5, 0.5, (len(k), 3))
    d[k] = unit(len(k))
    o[480, 0], o[481, 2], d[482, 1], d[483, 0] = np.nan, np.inf, np.nan, -np.inf
    d[484:488] = 0.0
    o[488:492, 1] = [np.nan, np.inf, -np.inf, np.nan]
    d[492:496, 2] = [np.inf, np.nan, np.inf, np.nan]
    # 496..511: from outside through the middle of the box
    k = np.arange(496, N_RAYS)
    o[k] = center + 2.5 * radius * unit(len(k))
    d[k] = (center + radius * rng.uniform(-0.3, 0.3, (len(k), 3))) - o[k]
    return o.astype(F), d.astype(F)


def reference_geometry(o_grid, d_grid, delta_scale, radii, dtype):
    """What the reference's classes give for the set-up's fp32 values, computed in ``dtype``."""
    t = lambda a: torch.from_numpy(np.asarray(a, F)).to(dtype)      # noqa: E731
    csi = ref_utils.ConcentricSpheresIntersector(t(np.array(RESO, F)), t(o_grid), t(d_grid), t(delta_scale))
    inner = (torch.cross(csi.origins, csi.dirs, dim=-1).norm(dim=-1) + 1e-3).clamp_min(1.0)
    out = {"origins": csi.origins.numpy(), "dirs": csi.dirs.numpy(), "world_step_scale": csi.world_step_scale.numpy(),
           "inner": inner.numpy()}
    ok_all, t_all, xy_all = [], [], []
    for r in radii:
        ok, tt = csi.intersect(float(r))
        pos = csi.origins + tt.unsqueeze(-1) * csi.dirs
        invr = 1.0 / pos.norm(dim=-1)
        xy = ref_utils.xyz2equirect(pos * invr.unsqueeze(-1), BG_RESO)
        ok_all.append(ok.numpy())
        t_all.append(tt.numpy())
        xy_all.append(xy.numpy())
    out.update(hit=np.stack(ok_all), t=np.stack(t_all), xy=np.stack(xy_all))
    return out


def main():
    rng = np.random.default_rng(20240917)
    links, density, sh = make_grid(rng, "bg", RESO, BASIS_DIM)
    density = (density * 3.0).astype(F)      # rays through a blob saturate
    grid = {"links": links, "density_data": density, "sh_data": sh, "radius": np.array(RADIUS, F), "center": np.array(CENTER, F)}
    o, d = make_rays(rng)
    all_radii = np.unique(np.concatenate([BO.radii(nl, st) for nl, st, _ in SETTINGS]))
    for attempt in range(100):      # a ray whose inner radius is within 1e-4 of a sphere's is drawn again
        og, dg, _, ds, _, _, ok = GO.ray_setup(grid, o, d)
        su = BO.setup(np.where(ok[:, None], og, 0), np.where(ok[:, None], dg, 1), np.where(ok, ds, 1), RESO, np.float64)
        close = ok & (np.abs(su["inner"][:, None] - all_radii[None, :].astype(np.float64)) < 1e-4).any(-1)
        if not close.any():
            break
        o2, d2 = make_rays(rng)
        o[close], d[close] = o2[close], d2[close]
    assert not close.any()
    out = {"links": links, "density": density, "sh": sh, "radius": np.array(RADIUS, F), "center": np.array(CENTER, F),
           "origins": o, "dirs": d, "setup_o": og, "setup_d": dg, "setup_delta_scale": ds, "setup_ok": ok,
           "brightness": np.float64(BRIGHTNESS), "settings": np.array(SETTINGS, dtype=np.float64),
           "geometry": np.array(GEOMETRY, dtype=np.float64)}
    bgs = {}
    for nl in NLAYERS:
        bl, bd = make_background(rng, nl)
        bgs[nl] = {"links": bl, "data": bd}
        out[f"bg{nl}_links"], out[f"bg{nl}_data"] = bl, bd
    for j, (nl, st) in enumerate(GEOMETRY):
        rr = BO.radii(nl, st)
        out[f"geo{j}_radii"] = rr
        for tag, dt in (("ref32", torch.float32), ("ref64", torch.float64)):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                geo = reference_geometry(np.where(ok[:, None], og, 0), np.where(ok[:, None], dg, 1), np.where(ok, ds, 1), rr, dt)
            for key, v in geo.items():
                if key in ("origins", "dirs", "world_step_scale", "inner"):
                    if j == 0:
                        out[f"{tag}_{key}"] = v
                else:
                    out[f"{tag}_geo{j}_{key}"] = v
    d_ref = d_ref_log = 0.0
    stats = dict(reach=0, stopped=0, dark=0, seam=0, outside=0, negative_t=0)
    su32 = BO.setup(np.where(ok[:, None], og, 0), np.where(ok[:, None], dg, 1), np.where(ok, ds, 1), RESO, F)
    stats["outside"] = int((ok & (np.sqrt(BO._dot(su32["O"], su32["O"])) > 1)).sum())
    stats["inner_above_1"] = int((ok & (su32["inner"] > 1)).sum())
    for j, (nl, st, stop) in enumerate(SETTINGS):
        fg_rgb, fg_logt = GO.render(grid, o, d, step_size=st, stop_thresh=stop, background_brightness=0.0)
        out[f"set{j}_fg_rgb"], out[f"set{j}_fg_logt"] = fg_rgb, fg_logt
        res = {}
        for T in (np.float32, np.float64):
            res[T] = BO.background_pass(og, dg, ds, ok, RESO, bgs[nl], fg_rgb, fg_logt, st, stop, BRIGHTNESS, T, return_stats=True)
        s32, s64 = res[np.float32][2], res[np.float64][2]
        assert (s32["stopped"] == s64["stopped"]).all(), "a ray stops in one precision only: choose other inputs"
        assert (s32["shaded"] == s64["shaded"]).all()
        dist = float(np.abs(res[np.float32][0].astype(np.float64) - res[np.float64][0]).max())
        dist_log = float(np.abs(res[np.float32][1].astype(np.float64) - res[np.float64][1]).max())
        d_ref, d_ref_log = max(d_ref, dist), max(d_ref_log, dist_log)
        reach = ok & ~s32["left_alone"] & (np.exp(fg_logt) > 0.5) & (s32["shaded"] > 0)
        stats["reach"] = max(stats["reach"], int(reach.sum()))
        stats["stopped"] = max(stats["stopped"], int(s32["stopped"].sum()))
        stats["dark"] = max(stats["dark"], int(s32["left_alone"].sum()))
        stats["seam"] = max(stats["seam"], int(s32["seam"].sum()))
        for r in BO.radii(nl, st):
            taken, t, _, _ = BO.hit(su32, r, F)
            stats["negative_t"] = max(stats["negative_t"], int((taken & ok & (t < 0)).sum()))
        print(f"setting {j} L={nl} step={st} stop={stop}: |fp32 - fp64| rgb {dist:.3e} log_T {dist_log:.3e}, reach {int(reach.sum())}, "
              f"stopped {int(s32['stopped'].sum())}, left alone {int(s32['left_alone'].sum())}, seam samples {int(s32['seam'].sum())}")
    print(stats)
    assert stats["reach"] >= 64 and stats["stopped"] >= 16 and stats["dark"] >= 16 and stats["seam"] >= 8
    assert stats["outside"] >= 32 and stats["inner_above_1"] >= 8 and stats["negative_t"] >= 8
    # d_ref: over colour and log_transmit, everything the pass returns; d_ref_rgb: the colour alone
    out["d_ref"], out["d_ref_rgb"] = np.float64(max(d_ref, d_ref_log)), np.float64(d_ref)
    path = os.path.join(HERE, "grid_background.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes", "d_ref", d_ref, d_ref_log)


if __name__ == "__main__":
    main()
