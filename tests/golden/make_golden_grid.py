"""Writes tests/golden/grid_render.npz: sparse voxel grids, rays, and what the reference's svox2 renders and samples from them.

    NERF_REFERENCE_SVOX2=/path/to/reference/svox2 python tests/golden/make_golden_grid.py

Runs on the CPU: ``svox2`` imports without its CUDA extension, and ``SparseGrid._volume_render_gradcheck_lerp`` /
``SparseGrid.sample(use_kernel=False)`` are pure PyTorch. Nothing of the reference is copied: the fixture holds arrays only
(grids and rays made here, the reference's outputs). Every render is recorded twice: in fp32 as the reference computes it,
and in fp64 (the same code on double tensors); ``d_ref`` = the largest |fp32 - fp64| over the rays of a grid is the
reference's own distance from exact arithmetic, and the tests allow 3x that.

The PyTorch statement has no ``sigma_thresh`` (it uses relu) and no early stop: it is the CUDA semantics at
``sigma_thresh = 0``, ``stop_thresh = 0``.
"""
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("NERF_REFERENCE_SVOX2")
if not REF:
    sys.exit("set NERF_REFERENCE_SVOX2 to the svox2 directory of the reference checkout (the one that holds svox2/svox2.py)")
sys.path.insert(0, REF)
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    import svox2  # noqa: E402  (reference)

# (name, reso, radius, center, basis_dim)
GRIDS = [
    ("a", (24, 20, 28), (1.0, 0.8, 1.2), (0.1, -0.2, 0.3), 9),
    ("b", (16, 16, 16), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), 4),
    ("c", (12, 14, 10), (0.5, 0.7, 0.6), (-0.3, 0.2, 0.0), 1),
    ("d", (64, 64, 64), (1.5, 1.5, 1.5), (0.0, 0.0, 0.0), 9),      # a single kept node
]
# (tag, background_brightness, step_size, near_clip)
VARIANTS = [("bg1", 1.0, 0.5, 0.0), ("bg0", 0.0, 0.5, 0.0), ("step", 1.0, 0.3, 0.0), ("near", 1.0, 0.5, 6.0)]
N_RAYS = 1024


def make_grid(rng, name, reso, basis_dim):
    """links / density / sh: about a fifth of the nodes kept in blobs, the outermost node layer empty, some empty links < -1,
    densities up to 40 (rays saturate), coefficients of both signs (the max(0, .) clamp is hit). Values are multiples of
    1/16 and 1/64 so that the file compresses."""
    X, Y, Z = reso
    if name == "d":
        kept = np.zeros(reso, dtype=bool)
        kept[30, 33, 31] = True
    else:
        i, j, k = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij")
        f = np.zeros(reso)
        for _ in range(6):
            w = rng.uniform(0.2, 0.9, 3)
            p = rng.uniform(0, 2 * np.pi, 3)
            f += np.sin(w[0] * i + p[0]) * np.sin(w[1] * j + p[1]) * np.sin(w[2] * k + p[2])
        interior = np.zeros(reso, dtype=bool)
        interior[1:-1, 1:-1, 1:-1] = True
        kept = (f > np.quantile(f[interior], 0.8)) & interior
    n = int(kept.sum())
    links = np.full(reso, -1, dtype=np.int32)
    links[kept] = rng.permutation(n).astype(np.int32)      # rows in no particular order
    empty = np.argwhere(~kept)
    pick = empty[rng.choice(len(empty), size=max(1, len(empty) // 10), replace=False)]
    links[pick[:, 0], pick[:, 1], pick[:, 2]] = rng.integers(-9, -1, len(pick)).astype(np.int32)      # arbitrary, not skip data
    density = np.round(rng.uniform(-4.0, 40.0, (n, 1)) * 16) / 16
    density[rng.random((n, 1)) < 0.1] = 0.0
    sh = np.round(rng.normal(0.0, 1.0, (n, 3 * basis_dim)) * 64) / 64
    if name == "d":
        density[:] = 25.0
    return links, density.astype(np.float32), sh.astype(np.float32)


def make_rays(rng, radius, center):
    radius, center = np.array(radius), np.array(center)
    n = N_RAYS
    o = np.empty((n, 3))
    d = np.empty((n, 3))
    # through the box from outside, non-unit directions
    k = np.arange(0, 704)
    u = rng.normal(size=(len(k), 3))
    o[k] = center + 3.0 * radius * u / np.linalg.norm(u, axis=-1, keepdims=True)
    target = center + radius * rng.uniform(-0.9, 0.9, (len(k), 3))
    d[k] = (target - o[k]) * rng.uniform(0.2, 5.0, (len(k), 1))
    # pointing away: miss the box
    k = np.arange(704, 800)
    u = rng.normal(size=(len(k), 3))
    o[k] = center + 3.0 * radius * u / np.linalg.norm(u, axis=-1, keepdims=True)
    d[k] = (o[k] - center) + rng.normal(size=(len(k), 3)) * 0.1
    # axis-parallel: one or two direction components exactly zero
    k = np.arange(800, 928)
    o[k] = center + radius * rng.uniform(-0.9, 0.9, (len(k), 3))
    d[k] = 0.0
    for r in k:
        ax = rng.integers(0, 3)
        sgn = rng.choice([-1.0, 1.0])
        d[r, ax] = sgn * rng.uniform(0.5, 2.0)
        o[r, ax] = center[ax] - sgn * 2.5 * radius[ax]
        if rng.random() < 0.5:
            d[r, (ax + 1) % 3] = rng.uniform(-0.3, 0.3)
    # origins inside the grid
    k = np.arange(928, n)
    o[k] = center + radius * rng.uniform(-0.8, 0.8, (len(k), 3))
    u = rng.normal(size=(len(k), 3))
    d[k] = u * rng.uniform(0.5, 2.0, (len(k), 1))
    return o.astype(np.float32), d.astype(np.float32)


def ref_grid(reso, radius, center, basis_dim, links, density, sh, dtype):
    g = svox2.SparseGrid(reso=[2, 2, 2], radius=list(radius), center=list(center), basis_dim=basis_dim, device="cpu")
    g.links = torch.from_numpy(links)
    g.density_data = torch.nn.Parameter(torch.from_numpy(density).to(dtype), requires_grad=False)
    g.sh_data = torch.nn.Parameter(torch.from_numpy(sh).to(dtype), requires_grad=False)
    g.capacity = density.shape[0]
    if dtype == torch.float64:
        g.radius = torch.tensor(np.array(radius, dtype=np.float32)).double()
        g.center = torch.tensor(np.array(center, dtype=np.float32)).double()
        g._offset = 0.5 * (1.0 - g.center / g.radius)
        g._scaling = 0.5 / g.radius

        def fetch64(self, lk):      # rows of the (double) data at the links, zeros at empty nodes
            present = (lk >= 0).unsqueeze(-1)
            rows = lk.clamp(min=0).long()
            zero = torch.zeros((), dtype=self.density_data.dtype)
            return torch.where(present, self.density_data[rows], zero), torch.where(present, self.sh_data[rows], zero)
        g._fetch_links = types.MethodType(fetch64, g)
    return g


def main():
    rng = np.random.default_rng(20240611)
    out = {}
    for name, reso, radius, center, basis_dim in GRIDS:
        links, density, sh = make_grid(rng, name, reso, basis_dim)
        o, d = make_rays(rng, radius, center)
        if name == "d":      # aim a part of the rays at the one kept node
            node = np.array(center) - np.array(radius) + (np.array([30, 33, 31]) + 0.5) * 2 * np.array(radius) / np.array(reso)
            d[:256] = ((node + rng.normal(size=(256, 3)) * 0.01 - o[:256]) * rng.uniform(0.5, 2.0, (256, 1))).astype(np.float32)
        out.update({f"{name}_links": links, f"{name}_density": density, f"{name}_sh": sh, f"{name}_origins": o,
                    f"{name}_dirs": d, f"{name}_radius": np.array(radius, np.float32),
                    f"{name}_center": np.array(center, np.float32)})
        g32 = ref_grid(reso, radius, center, basis_dim, links, density, sh, torch.float32)
        g64 = ref_grid(reso, radius, center, basis_dim, links, density, sh, torch.float64)
        d_ref = 0.0
        variants = VARIANTS if name == "a" else VARIANTS[:2]
        for tag, bg, step, near in variants:
            res = []
            for g, dt in ((g32, torch.float32), (g64, torch.float64)):
                g.opt.background_brightness, g.opt.step_size, g.opt.near_clip = bg, step, near
                torch.set_default_dtype(dt)
                with torch.no_grad():
                    rays = svox2.Rays(torch.from_numpy(o).to(dt), torch.from_numpy(d).to(dt))
                    res.append(g._volume_render_gradcheck_lerp(rays).numpy())
                torch.set_default_dtype(torch.float32)
            assert res[0].dtype == np.float32 and res[1].dtype == np.float64
            out[f"{name}_{tag}_rgb"] = res[0]
            out[f"{name}_{tag}_rgb64"] = res[1]
            dist = float(np.abs(res[0].astype(np.float64) - res[1]).max())
            d_ref = max(d_ref, dist)
            print(f"grid {name} {tag}: |fp32 - fp64| max {dist:.3e}, rays != background "
                  f"{int((np.abs(res[0] - bg).max(-1) > 1e-3).sum())}, saturated {int((res[0].max(-1) > bg + 0.5).sum())}")
        out[f"{name}_variants"] = np.array([[bg, step, near] for _, bg, step, near in variants], dtype=np.float64)
        out[f"{name}_d_ref"] = np.float64(d_ref)
        # sample(): world and grid coordinates, points inside, on and beyond the border
        pw = (np.array(center) + np.array(radius) * rng.uniform(-1.2, 1.2, (512, 3))).astype(np.float32)
        pg = (rng.uniform(-1.5, 1.0, (512, 3)) + rng.uniform(0, 1, (512, 1)) * np.array(reso)).astype(np.float32)
        with torch.no_grad():
            sw = g32.sample(torch.from_numpy(pw.copy()), use_kernel=False)
            sg = g32.sample(torch.from_numpy(pg.copy()), use_kernel=False, grid_coords=True)
        out.update({f"{name}_pts_world": pw, f"{name}_pts_grid": pg, f"{name}_sample_world_density": sw[0].numpy(),
                    f"{name}_sample_world_sh": sw[1].numpy(), f"{name}_sample_grid_density": sg[0].numpy(),
                    f"{name}_sample_grid_sh": sg[1].numpy()})
    # a small camera: off-centre principal point, fx != fy, a rotated pose
    ang = np.array([0.3, -0.5, 0.2])
    rx = np.array([[1, 0, 0], [0, np.cos(ang[0]), -np.sin(ang[0])], [0, np.sin(ang[0]), np.cos(ang[0])]])
    ry = np.array([[np.cos(ang[1]), 0, np.sin(ang[1])], [0, 1, 0], [-np.sin(ang[1]), 0, np.cos(ang[1])]])
    rz = np.array([[np.cos(ang[2]), -np.sin(ang[2]), 0], [np.sin(ang[2]), np.cos(ang[2]), 0], [0, 0, 1]])
    c2w = np.concatenate([rz @ ry @ rx, np.array([[0.4], [-2.9], [1.1]])], 1).astype(np.float32)
    cam = svox2.Camera(torch.from_numpy(c2w), fx=30.0, fy=28.0, cx=11.3, cy=8.6, width=24, height=16)
    rays = cam.gen_rays()
    out.update({"cam_c2w": c2w, "cam_intrinsics": np.array([30.0, 28.0, 11.3, 8.6]), "cam_size": np.array([24, 16]),
                "cam_origins": rays.origins.numpy(), "cam_dirs": rays.dirs.numpy()})
    path = os.path.join(HERE, "grid_render.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
