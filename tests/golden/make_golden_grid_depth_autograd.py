"""Writes tests/golden/grid_depth_autograd.npz: what the reference's svox2 gives, through PyTorch autograd on the CPU, for
the gradients of depth and transmittance with respect to ``density_data``.

    NERF_REFERENCE_SVOX2=/path/to/reference/svox2 python tests/golden/make_golden_grid_depth_autograd.py

The reference has no differentiable depth; its PyTorch renderer (``_volume_render_gradcheck_lerp``) is differentiable in the
colour only. Depth and transmittance are therefore taken out of the renderer as make_golden_grid_depth.py takes them, with
the renders kept under autograd: on grid "e" of tests/golden/grid_depth.npz (dense, ``basis_dim`` 1, 12 x 10 x 14, the colour
of a node is its position), with c0 / c1 the renders at background brightness 0 / 1,
``T = mean(c1 - c0)`` and ``depth = ((c0 size - (1 - T) o_grid) . d_grid) delta_scale``. The PyTorch renderer has no
``sigma_thresh`` and no early stop: this is the semantics at ``sigma_thresh = 0``, ``stop_thresh = 0``. The reference never
takes a gradient of ``log T`` itself - ``log(c1 - c0)`` is meaningless in fp32 where T reaches 1e-11 - so that cotangent is
anchored through ``T = exp(log T)`` in (ii) - (iv). Every loss once through the fp32 and once through the fp64 renderer (the
derivation after the renders is in fp64 for both, as in make_golden_grid_depth.py: what differs is the renderer's forward and
backward); stored are the fp64
gradient rounded to fp32 and ``d_ref`` = max |fp32 gradient - fp64 gradient| from the unrounded values: the reference's own
distance from exact arithmetic. Nothing of the reference is copied: the fixture holds arrays only.

(i)   ``sum(w * depth)`` with a seeded normal ``w`` (stored, rounded to multiples of 1/64), grid e          -> ``e_i_*``
(ii)  ``sum(w2 * T)`` with a second such ``w2``, grid e                                                   -> ``e_ii_*``
(iii) ``mean((depth / (1 - T + 1e-3) - 1) ** 2) + 0.1 mean(T (1 - T))``, grid e                           -> ``e_iii_*``
(iv)  loss (ii) on the sparse grids a, b, c and the rays of tests/golden/grid_render.npz (their colours are arbitrary:
      T = mean(c1 - c0) needs no colour coding)                                                           -> ``{a,b,c}_iv_*``

The bar of the tests is max(3 d_ref, 1e-5 max |g64|) per entry. So that this bar cannot hide a failure, every recorded
gradient must satisfy 3 d_ref <= 1e-2 max |g64| (asserted here; a sparse grid that fails is left out and named in the output).
That is a condition on the fixture, not on the code under test, and for (i) and (ii) it depends on the cotangent: the
derivation subtracts renders of order 1 to get a T down to 1e-11, the fp32 renderer's backward carries that cancellation, and
d_ref - a maximum over all entries - is set by the few rays where it is worst times their weight. Over the seeds 20240915,
20250630, 20251018 and 1 - 5, d_ref / max |g64| of (i) ranged from 3.1e-4 to 6.3e-3 and of (ii) from 3.0e-4 to 3.1e-3; (iii)
has no seeded weights and is 1.9e-3; (iv) is below 5e-6 on all of a, b, c. SEED = 1 is the first of 1, 2, 3, ... that keeps
(i) and (ii) inside the cap (2.1e-3 and 2.0e-3): the fixture then tests gradients, not the reference's fp32 noise.
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_grid as MG  # noqa: E402  (this project's; imports svox2 from NERF_REFERENCE_SVOX2)

svox2 = MG.svox2
E_RESO = (12, 10, 14)
CAP = 1e-2      # 3 d_ref <= CAP * max |g64|
EPS = 1e-3
SEED = 1      # of the cotangents; see the docstring


def renders(g, o, d, dtype):
    """(c0, c1): the renders at background brightness 0 and 1, under autograd"""
    g.opt.step_size, g.opt.near_clip = 0.5, 0.0
    rays = svox2.Rays(torch.from_numpy(o).to(dtype), torch.from_numpy(d).to(dtype))
    out = []
    for bg in (0.0, 1.0):
        g.opt.background_brightness = bg
        out.append(g._volume_render_gradcheck_lerp(rays))
    return out


def grad_of(make_grid, o, d, dtype, loss_of):
    g = make_grid(dtype)
    g.density_data.requires_grad_(True)
    torch.set_default_dtype(dtype)
    try:
        c0, c1 = renders(g, o, d, dtype)
        loss_of(c0, c1).backward()
    finally:
        torch.set_default_dtype(torch.float32)
    return g.density_data.grad.numpy().copy()


def record(out, prefix, make_grid, o, d, loss_of, label, must=True):
    g32 = grad_of(make_grid, o, d, torch.float32, lambda c0, c1: loss_of(c0, c1, torch.float32))
    g64 = grad_of(make_grid, o, d, torch.float64, lambda c0, c1: loss_of(c0, c1, torch.float64))
    assert g32.dtype == np.float32 and g64.dtype == np.float64
    d_ref, big = float(np.abs(g32.astype(np.float64) - g64).max()), float(np.abs(g64).max())
    ok = 3.0 * d_ref <= CAP * big
    print(f"{label}: max |g64| {big:.3e}, |fp32 - fp64| max {d_ref:.3e} = {d_ref / big:.2e} of it, rows != 0: "
          f"{int((g64 != 0).any(-1).sum())} of {g64.shape[0]}{'' if ok else '   ABOVE THE CAP: left out'}")
    assert ok or not must, (label, d_ref, big)
    if ok:
        out[f"{prefix}_grad64"] = g64.astype(np.float32)
        out[f"{prefix}_d_ref"] = np.float64(d_ref)
    return ok


def main():
    ze = np.load(os.path.join(HERE, "grid_depth.npz"))
    zr = np.load(os.path.join(HERE, "grid_render.npz"))
    rng = np.random.default_rng(SEED)
    out = {}
    # ---- grid e ----
    o, d = ze["e_origins"], ze["e_dirs"]
    n = o.shape[0]
    w = (np.round(rng.normal(0.0, 1.0, n) * 64) / 64).astype(np.float32)
    w2 = (np.round(rng.normal(0.0, 1.0, n) * 64) / 64).astype(np.float32)
    out["e_w"], out["e_w2"] = w, w2
    size = np.array(E_RESO, dtype=np.float64)
    radius, center = ze["e_radius"].astype(np.float64), ze["e_center"].astype(np.float64)
    o_grid = (0.5 * (1.0 - center / radius) * size - 0.5) + o.astype(np.float64) * (0.5 / radius * size)
    d_grid = d.astype(np.float64) / np.linalg.norm(d.astype(np.float64), axis=-1, keepdims=True) * (0.5 / radius * size)
    delta_scale = 1.0 / np.linalg.norm(d_grid, axis=-1)
    d_grid *= delta_scale[:, None]

    def grid_e(dtype):
        return MG.ref_grid(E_RESO, ze["e_radius"].tolist(), ze["e_center"].tolist(), 1, ze["e_links"], ze["e_density"], ze["e_sh"], dtype)

    def depth_and_t(c0, c1):
        """make_golden_grid_depth.py's derivation, in fp64 from the renders of either precision (as there)"""
        t = lambda a: torch.from_numpy(np.asarray(a, np.float64))      # noqa: E731
        c0, c1 = c0.double(), c1.double()
        T = (c1 - c0).mean(-1)
        wt = ((c0 * t(size) - (1.0 - T)[:, None] * t(o_grid)) * t(d_grid)).sum(-1)
        return wt * t(delta_scale), T

    def loss_i(c0, c1, dtype):
        return (torch.from_numpy(w).double() * depth_and_t(c0, c1)[0]).sum()

    def loss_ii(c0, c1, dtype, weights=w2):
        return (torch.from_numpy(weights).double() * (c1.double() - c0.double()).mean(-1)).sum()

    def loss_iii(c0, c1, dtype):
        depth, T = depth_and_t(c0, c1)
        return ((depth / (1.0 - T + EPS) - 1.0) ** 2).mean() + 0.1 * (T * (1.0 - T)).mean()

    record(out, "e_i", grid_e, o, d, loss_i, "(i) grid e")
    record(out, "e_ii", grid_e, o, d, loss_ii, "(ii) grid e")
    record(out, "e_iii", grid_e, o, d, loss_iii, "(iii) grid e")
    # ---- (iv) the sparse grids ----
    kept = []
    for name in ("a", "b", "c"):
        _, reso, radius_, center_, basis_dim = next(s for s in MG.GRIDS if s[0] == name)
        oo, dd = zr[f"{name}_origins"], zr[f"{name}_dirs"]
        ww = (np.round(rng.normal(0.0, 1.0, oo.shape[0]) * 64) / 64).astype(np.float32)

        def grid_s(dtype):
            return MG.ref_grid(reso, radius_, center_, basis_dim, zr[f"{name}_links"], zr[f"{name}_density"], zr[f"{name}_sh"], dtype)

        if record(out, f"{name}_iv", grid_s, oo, dd, lambda c0, c1, dtype: loss_ii(c0, c1, dtype, ww), f"(iv) grid {name}", must=False):
            out[f"{name}_w2"] = ww
            kept.append(name)
    assert kept, "no sparse grid stays inside the cap"
    out["eps"] = np.float64(EPS)
    path = os.path.join(HERE, "grid_depth_autograd.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; sparse grids kept:", kept)
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        main()
