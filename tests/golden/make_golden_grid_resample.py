"""Writes tests/golden/grid_resample.npz: what the reference's ``SparseGrid.resample`` makes of the fixture grids.

    NERF_REFERENCE_SVOX2=/path/to/reference/svox2 python tests/golden/make_golden_grid_resample.py

Runs on the CPU, where ``svox2`` imports without its CUDA extension: ``resample`` is called with ``dilate=0, cameras=None,
accelerate=False`` (``_C.dilate`` and ``_C.grid_weight_render`` do not exist there) and its ``sample`` falls back to PyTorch.
Nothing of the reference is copied: the fixture holds arrays only. The grids are those of make_golden_grid.py (read from
grid_render.npz: values that are multiples of 1/16 and 1/64, rows in permuted order). Every case is run twice: in fp32 as the
reference computes it, and in fp64 (the same code on double tables with the ``fetch64`` patch of make_golden_grid.py and the
lattice points widened to double before ``sample``). Stored per case: the fp32 ``links`` / ``density_data`` / ``sh_data``, the
fp64 mask (bit-packed), and ``d_ref`` = max |fp32 - fp64| per table over the nodes both kept - the reference's own distance
from exact arithmetic; the tests allow 3x that.
"""
import contextlib
import io
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

# (case, source grid, target resolution, sigma_thresh): 2x up, a non-integer ratio up, one down, the same resolution
CASES = [
    ("b_x2", "b", (32, 32, 32), 5.0),
    ("c_x2", "c", (24, 28, 20), 5.0),
    ("b_x1p5", "b", (24, 24, 24), 5.0),
    ("c_odd", "c", (17, 23, 13), 5.0),
    ("a_odd", "a", (29, 23, 33), 5.0),
    ("a_down", "a", (16, 13, 19), 5.0),
    ("b_down", "b", (9, 11, 10), 2.0),
    ("a_same", "a", (24, 20, 28), 5.0),
    ("c_same", "c", (12, 14, 10), 0.5),
]


def ref_grid(links, density, sh, radius, center, dtype):
    basis_dim = sh.shape[1] // 3
    g = svox2.SparseGrid(reso=[2, 2, 2], radius=list(radius), center=list(center), basis_dim=basis_dim, device="cpu")
    g.links = torch.from_numpy(links.copy())
    g.density_data = torch.nn.Parameter(torch.from_numpy(density).to(dtype), requires_grad=False)
    g.sh_data = torch.nn.Parameter(torch.from_numpy(sh).to(dtype), requires_grad=False)
    g.capacity = density.shape[0]
    if dtype == torch.float64:
        def fetch64(self, lk):      # rows of the (double) data at the links, zeros at empty nodes
            present = (lk >= 0).unsqueeze(-1)
            rows = lk.clamp(min=0).long()
            zero = torch.zeros((), dtype=self.density_data.dtype)
            return torch.where(present, self.density_data[rows], zero), torch.where(present, self.sh_data[rows], zero)
        g._fetch_links = types.MethodType(fetch64, g)
        plain = g.sample

        def sample64(points, **kw):      # the fp32 lattice points, widened: weights and interpolation in double
            return plain(points.double(), **kw)
        g.sample = sample64
    return g


def run(g, reso, sigma_thresh):
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        g.resample(list(reso), sigma_thresh=sigma_thresh, dilate=0, cameras=None, accelerate=False)
    return g.links.numpy().astype(np.int32), g.density_data.detach().numpy(), g.sh_data.detach().numpy()


def main():
    z = np.load(os.path.join(HERE, "grid_render.npz"))
    out = {"cases": np.array([c[0] for c in CASES]), "sources": np.array([c[1] for c in CASES]),
           "resos": np.array([c[2] for c in CASES], dtype=np.int32), "sigma_thresh": np.array([c[3] for c in CASES])}
    for case, name, reso, thresh in CASES:
        src = [z[f"{name}_{k}"] for k in ("links", "density", "sh", "radius", "center")]
        l32, d32, s32 = run(ref_grid(*src, torch.float32), reso, thresh)
        l64, d64, s64 = run(ref_grid(*src, torch.float64), reso, thresh)
        assert d32.dtype == np.float32 and s32.dtype == np.float32 and d64.dtype == np.float64 and s64.dtype == np.float64
        m32, m64 = l32 >= 0, l64 >= 0
        both = m32 & m64
        dd = np.abs(d32[l32[both]].astype(np.float64) - d64[l64[both]])
        ds = np.abs(s32[l32[both]].astype(np.float64) - s64[l64[both]])
        d_ref = np.array([dd.max() if dd.size else 0.0, ds.max() if ds.size else 0.0])
        out.update({f"{case}_links": l32, f"{case}_density": d32, f"{case}_sh": s32,
                    f"{case}_mask64": np.packbits(m64.reshape(-1)), f"{case}_d_ref": d_ref})
        print(f"{case}: {name} {tuple(l32.shape)}, thresh {thresh}: kept {int(m32.sum())} of {m32.size}, mask flips fp32/fp64 "
              f"{int((m32 != m64).sum())}, d_ref density {d_ref[0]:.3e} sh {d_ref[1]:.3e}, max |density| {np.abs(d64).max():.3f}, "
              f"max |sh| {np.abs(s64).max() if s64.size else 0.0:.3f}")
    path = os.path.join(HERE, "grid_resample.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
