"""Writes tests/golden/grid_train.npz: what the reference's svox2 gives for the gradients of the MSE loss through its renderer,
and for a short RMSProp loop, on the grids and rays of tests/golden/grid_render.npz.

    NERF_REFERENCE_SVOX2=/path/to/reference/svox2 python tests/golden/make_golden_grid_train.py

Runs on the CPU in seconds: PyTorch autograd through ``SparseGrid._volume_render_gradcheck_lerp`` (the CUDA semantics at
``sigma_thresh = 0``, ``stop_thresh = 0``), once on fp32 and once on fp64 tensors. Nothing of the reference is copied: the
fixture holds arrays only.

(a) gradients. Per grid a-d and background 1 / 0: ``loss = mean((rgb - gt) ** 2)`` with a seeded uniform ``gt``; the fp64
    gradients with respect to ``density_data`` and ``sh_data`` are stored (rounded to fp32 for the size of the file: a
    relative 6e-8, far below every bar), and ``d_ref`` = max |fp32 gradient - fp64 gradient| per tensor, computed here from
    the unrounded values, is the reference's own distance from exact arithmetic.
(b) a 20-iteration loop on grids b and c from ``0.5 * density`` and zero SH towards the recorded ``bg1_rgb64`` of the first 704
    rays, 256 seeded rays per iteration, masked RMSProp as include/nerf_mi355x.h states it (beta 0.95, eps 1e-8,
    lr_sh 1e-2, lr_sigma 1.0) on the rows whose gradient is not zero. Losses, final tables and the per-iteration masks.
    lr_sigma is 1.0, not svox2's 30: at 30 the first steps are +-30 by the sign of the gradient and the two precisions end
    8-16 apart in density - a fixture of noise.
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
N_ITERS, N_BATCH, N_POOL = 20, 256, 704
BETA, EPS, LR_SH, LR_SIGMA = 0.95, 1e-8, 1e-2, 1.0


def grid_for(z, name, dtype, density=None, sh=None):
    spec = next(s for s in MG.GRIDS if s[0] == name)
    _, reso, radius, center, basis_dim = spec
    density = z[f"{name}_density"] if density is None else density
    sh = z[f"{name}_sh"] if sh is None else sh
    g = MG.ref_grid(reso, radius, center, basis_dim, z[f"{name}_links"], density, sh, dtype)
    g.density_data.requires_grad_(True)
    g.sh_data.requires_grad_(True)
    return g


def loss_and_grads(g, o, d, gt, bg, dtype):
    """loss, d loss / d density_data, d loss / d sh_data as numpy in `dtype`"""
    g.opt.background_brightness, g.opt.step_size, g.opt.near_clip = bg, 0.5, 0.0
    g.density_data.grad = None
    g.sh_data.grad = None
    torch.set_default_dtype(dtype)
    try:
        rays = svox2.Rays(torch.from_numpy(o).to(dtype), torch.from_numpy(d).to(dtype))
        rgb = g._volume_render_gradcheck_lerp(rays)
        loss = ((rgb - torch.from_numpy(gt).to(dtype)) ** 2).mean()
        loss.backward()
    finally:
        torch.set_default_dtype(torch.float32)
    return loss.item(), g.density_data.grad.numpy().copy(), g.sh_data.grad.numpy().copy()


def rmsprop(data, rms, grad, mask, lr):
    """in place, on the masked rows; the statement of include/nerf_mi355x.h in the tensors' own precision"""
    dt = data.dtype
    g = grad[mask]
    g2 = g * g
    r = rms[mask]
    r = torch.where(r == 0, g2, g2 + torch.tensor(BETA, dtype=dt) * (r - g2))
    rms[mask] = r
    upd = (torch.tensor(lr, dtype=dt) * g) / (torch.sqrt(r) + torch.tensor(EPS, dtype=dt))
    data[mask] = torch.clamp_min(data[mask] - upd, torch.tensor(-1e9, dtype=dt))


def main():
    z = np.load(os.path.join(HERE, "grid_render.npz"))
    rng = np.random.default_rng(20250117)
    out = {}
    # ---- (a) ----
    for name in ("a", "b", "c", "d"):
        o, d = z[f"{name}_origins"], z[f"{name}_dirs"]
        gt = rng.uniform(0.0, 1.0, (o.shape[0], 3)).astype(np.float32)
        out[f"{name}_rgb_gt"] = gt
        for tag, bg in (("bg1", 1.0), ("bg0", 0.0)):
            l32, gd32, gs32 = loss_and_grads(grid_for(z, name, torch.float32), o, d, gt, bg, torch.float32)
            l64, gd64, gs64 = loss_and_grads(grid_for(z, name, torch.float64), o, d, gt, bg, torch.float64)
            assert gd32.dtype == np.float32 and gd64.dtype == np.float64
            out[f"{name}_{tag}_grad_density64"] = gd64.astype(np.float32)
            out[f"{name}_{tag}_grad_sh64"] = gs64.astype(np.float32)
            out[f"{name}_{tag}_loss64"] = np.float64(l64)
            for key, a32, a64 in (("density", gd32, gd64), ("sh", gs32, gs64)):
                d_ref = float(np.abs(a32.astype(np.float64) - a64).max())
                out[f"{name}_{tag}_grad_{key}_d_ref"] = np.float64(d_ref)
                print(f"grid {name} {tag} d/d{key}: max |g64| {np.abs(a64).max():.3e}, |fp32 - fp64| max {d_ref:.3e} "
                      f"= {d_ref / np.abs(a64).max():.2e} of it, rows != 0: {int((a64 != 0).any(-1).sum())} of {a64.shape[0]}")
    # ---- (b) ----
    for name in ("b", "c"):
        o, d = z[f"{name}_origins"][:N_POOL], z[f"{name}_dirs"][:N_POOL]
        target = z[f"{name}_bg1_rgb64"][:N_POOL]
        idx = np.stack([rng.choice(N_POOL, N_BATCH, replace=False) for _ in range(N_ITERS)]).astype(np.int32)
        out[f"{name}_loop_idx"] = idx
        res = {}
        for dtype, tagd in ((torch.float32, "32"), (torch.float64, "64")):
            npdt = np.float32 if dtype == torch.float32 else np.float64
            g = grid_for(z, name, dtype, (0.5 * z[f"{name}_density"]).astype(np.float32), np.zeros_like(z[f"{name}_sh"]))
            rms_d = torch.zeros_like(g.density_data.data)
            rms_s = torch.zeros_like(g.sh_data.data)
            losses, masks = [], []
            for it in range(N_ITERS):
                k = idx[it]
                loss, gd, gs = loss_and_grads(g, o[k], d[k], target[k].astype(npdt), 1.0, dtype)
                mask = torch.from_numpy((gd != 0).any(-1) | (gs != 0).any(-1))
                with torch.no_grad():
                    rmsprop(g.density_data.data, rms_d, torch.from_numpy(gd), mask, LR_SIGMA)
                    rmsprop(g.sh_data.data, rms_s, torch.from_numpy(gs), mask, LR_SH)
                losses.append(loss)
                masks.append(mask.numpy())
            res[tagd] = (np.array(losses, dtype=np.float64), g.density_data.data.numpy().copy(), g.sh_data.data.numpy().copy(),
                         np.stack(masks))
        l32, d32, s32, m32 = res["32"]
        l64, d64, s64, m64 = res["64"]
        out.update({f"{name}_loop_loss32": l32, f"{name}_loop_loss64": l64, f"{name}_loop_density32": d32,
                    f"{name}_loop_density64": d64, f"{name}_loop_sh32": s32, f"{name}_loop_sh64": s64,
                    f"{name}_loop_mask64": np.packbits(m64, axis=-1), f"{name}_loop_params": np.array([BETA, EPS, LR_SH, LR_SIGMA])})
        dl = float(np.abs(l32 - l64).max())
        print(f"grid {name} loop: loss {l64[0]:.4f} -> {l64[-1]:.4f}, max |l32 - l64| {dl:.2e}, final density |32 - 64| max "
              f"{np.abs(d32 - d64).max():.2e}, sh {np.abs(s32 - s64).max():.2e}, masks equal {bool((m32 == m64).all())}, "
              f"rows per step {m64.sum(-1).min()}..{m64.sum(-1).max()} of {m64.shape[1]}")
        # the fixture must test the optimisation, not noise
        assert dl < 1e-3 * (l64[0] - l64[-1]), (name, dl, l64[0] - l64[-1])
    path = os.path.join(HERE, "grid_train.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        main()
