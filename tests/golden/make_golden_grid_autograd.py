"""Writes tests/golden/grid_autograd.npz: what the reference's svox2 gives, through PyTorch autograd on the CPU, for the
gradients a differentiable grid must deliver, on the grids and rays of tests/golden/grid_render.npz.

    NERF_REFERENCE_SVOX2=/path/to/reference/svox2 python tests/golden/make_golden_grid_autograd.py

Per grid a-d, every quantity once on fp32 and once on fp64 tensors; stored are the fp64 gradients with respect to
``density_data`` and ``sh_data`` rounded to fp32 (a relative 6e-8, far below every bar) and ``d_ref`` = max |fp32 gradient -
fp64 gradient| per tensor, computed from the unrounded values: the reference's own distance from exact arithmetic.
Nothing of the reference is copied: the fixture holds arrays only.

(i)   the render's vector-Jacobian product itself: ``loss = (rgb * w).sum()`` with a seeded normal ``w [N, 3]`` (stored,
      rounded to multiples of 1/64) through ``_volume_render_gradcheck_lerp``, at background 1 and 0     -> ``*_vjp_*``
      With ``w`` fixed the SH gradient, ``weight * Y_k * w_c`` at every sample, does not depend on the background: it is
      checked to be the same array at both and stored once, as ``{grid}_vjp_grad_sh64`` (the file has to stay under 1 MiB).
(ii)  a loss that is not the fused kernel's: Charbonnier, ``mean(sqrt((rgb - gt) ** 2 + 1e-3))`` with the ``rgb_gt`` of
      grid_train.npz, at background 1 and 0                                                              -> ``*_charb_*``
(iii) the sampler's transpose: the gradients of ``(sigma * cd).sum() + (sh * cs).sum()`` through
      ``sample(use_kernel=False, grid_coords=True)`` at the fixture's ``*_pts_grid`` with seeded normal ``cd``, ``cs``
      (stored, rounded to multiples of 1/16)                                                             -> ``*_sample_*``
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_grid_train as MT  # noqa: E402  (this project's; imports svox2 from NERF_REFERENCE_SVOX2)

svox2 = MT.svox2
CHARB_EPS = 1e-3


def render_grads(g, o, d, loss_of, bg, dtype):
    g.opt.background_brightness, g.opt.step_size, g.opt.near_clip = bg, 0.5, 0.0
    torch.set_default_dtype(dtype)
    try:
        rays = svox2.Rays(torch.from_numpy(o).to(dtype), torch.from_numpy(d).to(dtype))
        loss_of(g._volume_render_gradcheck_lerp(rays)).backward()
    finally:
        torch.set_default_dtype(torch.float32)
    return g.density_data.grad.numpy().copy(), g.sh_data.grad.numpy().copy()


def sample_grads(g, pts, cd, cs, dtype):
    torch.set_default_dtype(dtype)
    try:
        sigma, sh = g.sample(torch.from_numpy(pts.copy()).to(dtype), use_kernel=False, grid_coords=True)
        ((sigma * torch.from_numpy(cd).to(dtype)).sum() + (sh * torch.from_numpy(cs).to(dtype)).sum()).backward()
    finally:
        torch.set_default_dtype(torch.float32)
    return g.density_data.grad.numpy().copy(), g.sh_data.grad.numpy().copy()


def record(out, prefix, g32, g64, label, keys=("density", "sh")):
    for key, a32, a64 in (("density", g32[0], g64[0]), ("sh", g32[1], g64[1])):
        if key not in keys:
            continue
        assert a32.dtype == np.float32 and a64.dtype == np.float64
        d_ref = float(np.abs(a32.astype(np.float64) - a64).max())
        out[f"{prefix}_grad_{key}64"] = a64.astype(np.float32)
        out[f"{prefix}_grad_{key}_d_ref"] = np.float64(d_ref)
        print(f"{label} d/d{key}: max |g64| {np.abs(a64).max():.3e}, |fp32 - fp64| max {d_ref:.3e} = "
              f"{d_ref / np.abs(a64).max():.2e} of it, rows != 0: {int((a64 != 0).any(-1).sum())} of {a64.shape[0]}")


def main():
    z = np.load(os.path.join(HERE, "grid_render.npz"))
    t = np.load(os.path.join(HERE, "grid_train.npz"))
    rng = np.random.default_rng(20250630)
    out = {}
    for name in ("a", "b", "c", "d"):
        o, d, gt = z[f"{name}_origins"], z[f"{name}_dirs"], t[f"{name}_rgb_gt"]
        w = (np.round(rng.normal(0.0, 1.0, (o.shape[0], 3)) * 64) / 64).astype(np.float32)
        out[f"{name}_vjp_w"] = w
        for tag, bg in (("bg1", 1.0), ("bg0", 0.0)):
            res = {}
            for dtype in (torch.float32, torch.float64):
                vjp = render_grads(MT.grid_for(z, name, dtype), o, d, lambda rgb: (rgb * torch.from_numpy(w).to(dtype)).sum(),
                                   bg, dtype)
                charb = render_grads(MT.grid_for(z, name, dtype), o, d,
                                     lambda rgb: torch.sqrt((rgb - torch.from_numpy(gt).to(dtype)) ** 2 + CHARB_EPS).mean(),
                                     bg, dtype)
                res[dtype] = (vjp, charb)
            record(out, f"{name}_{tag}_vjp", res[torch.float32][0], res[torch.float64][0], f"(i) grid {name} {tag}", ("density",))
            if tag == "bg1":
                record(out, f"{name}_vjp", res[torch.float32][0], res[torch.float64][0], f"(i) grid {name} both", ("sh",))
                vjp_sh = [res[dt][0][1] for dt in (torch.float32, torch.float64)]
            else:
                assert all(np.array_equal(a, res[dt][0][1]) for a, dt in zip(vjp_sh, (torch.float32, torch.float64)))
            record(out, f"{name}_{tag}_charb", res[torch.float32][1], res[torch.float64][1], f"(ii) grid {name} {tag}")
        pts = z[f"{name}_pts_grid"]
        cols = z[f"{name}_sh"].shape[1]
        cd = (np.round(rng.normal(0.0, 1.0, (pts.shape[0], 1)) * 16) / 16).astype(np.float32)
        cs = (np.round(rng.normal(0.0, 1.0, (pts.shape[0], cols)) * 16) / 16).astype(np.float32)
        out[f"{name}_sample_cd"], out[f"{name}_sample_cs"] = cd, cs
        res = [sample_grads(MT.grid_for(z, name, dtype), pts, cd, cs, dtype) for dtype in (torch.float32, torch.float64)]
        record(out, f"{name}_sample", res[0], res[1], f"(iii) grid {name}")
    out["charb_eps"] = np.float64(CHARB_EPS)
    path = os.path.join(HERE, "grid_autograd.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        main()
