"""Writes tests/golden/grid_train_losses.npz: what the reference's svox2 gives for the gradients of the MSE loss plus its two
regularisers (the beta loss on a ray's final transmittance, the Cauchy sparsity loss on the sampled densities) through its
renderer, and for a short RMSProp loop with both on, on the grids and rays of tests/golden/grid_render.npz and the targets of
tests/golden/grid_train.npz.

    NERF_REFERENCE_SVOX2=/path/to/reference/svox2 python tests/golden/make_golden_grid_train_losses.py

Runs on the CPU in a minute: PyTorch autograd through ``SparseGrid._volume_render_gradcheck_lerp`` (the CUDA semantics at
``sigma_thresh = 0``, ``stop_thresh = 0``), once on fp32 and once on fp64 tensors. Nothing of the reference is copied: the
fixture holds arrays only.

    loss = mean((rgb - gt) ** 2) + (lambda_beta / n) * sum_ray [log_T + log(1 - exp(log_T) + 1e-3)]
                                 + lambda_sparsity * sum over samples of log(1 + 2 sigma ** 2)

whose derivatives with respect to ``log_T`` and ``sigma`` are the two factors of the CUDA kernel (and of
include/nerf_mi355x.h, nerf_grid_fused_backward_losses). Where the two quantities are taken, both by hooks that stand in
the renderer's own calls while it runs and change no value it computes:
  log_T   where the renderer multiplies ``exp(log_T)`` by ``opt.background_brightness``: the brightness is an object whose
          ``__rmul__`` receives that product's left operand; ``torch.exp`` is wrapped meanwhile and remembers its last
          argument, which is ``log_T`` itself (checked: its exp is the operand, bit for bit). The transmittance alone would not
          do: it underflows to 0 on the dense rays of these grids and its logarithm has no gradient there.
  sigma   where the renderer calls ``torch.relu`` on it: the wrapped ``torch.relu`` keeps every result. A sample with
          sigma <= 0 has relu 0, adds log(1) = 0 and has no gradient: it is not counted, as in the kernel at sigma_thresh = 0.

(a) gradients. Per grid a-d, background 1 / 0 and the three settings (beta, sparsity) = (on, 0), (0, on), (on, on): the fp64
    gradient with respect to ``density_data`` (rounded to fp32 for the size of the file) and ``d_ref`` = max |fp32 gradient -
    fp64 gradient| for both tables, from the unrounded values. The gradient with respect to ``sh_data`` does not depend on the
    weights: it is grid_train.npz's (asserted here), so only its ``d_ref`` is stored.
    The weights are per grid, chosen so that each term alone moves ``grad_density`` by between 10 % and 90 % of its norm (the
    published 1e-5 and 1e-11 vanish in fp32 next to the MSE gradient on these grids); ``share`` = |g(term on) - g(terms off)| /
    |g(terms off)| in the 2-norm (fp64) is asserted and recorded.
(b) the 20-iteration loop of make_golden_grid_train.py (grids b and c, 256 of the first 704 rays per iteration by that
    fixture's own ``loop_idx``, masked RMSProp, lr_sigma 1.0) with both terms on. Losses (the MSE part, which is what a training
    step reports), final tables and the per-iteration masks.
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
# name -> (lambda_beta, lambda_sparsity)
WEIGHTS = {"a": (0.008, 1e-6), "b": (0.005, 1e-6), "c": (0.012, 1.5e-6), "d": (0.09, 2e-6)}
SETTINGS = (("beta", 1, 0), ("sparsity", 0, 1), ("both", 1, 1))


class Brightness:
    """Stands where the renderer reads ``opt.background_brightness``: it is true, and ``exp(log_T).unsqueeze(-1) * self`` is
    that operand times the real brightness, after ``log_T`` has been taken from the wrapped ``torch.exp``."""

    def __init__(self, value, taps):
        self.value, self.taps = value, taps

    def __bool__(self):
        return True

    def __rmul__(self, t):
        log_t = self.taps["exp_arg"]
        assert torch.equal(torch.exp(log_t).unsqueeze(-1), t)
        self.taps["log_t"] = log_t
        return t * self.value


class Taps:
    """While active, ``torch.exp`` remembers its last argument and ``torch.relu`` keeps every result."""

    def __enter__(self):
        self.d = {"relu": []}
        self.exp, self.relu = torch.exp, torch.relu
        d, exp, relu = self.d, self.exp, self.relu

        def tap_exp(x):
            d["exp_arg"] = x
            return exp(x)

        def tap_relu(x):
            y = relu(x)
            d["relu"].append(y)
            return y

        torch.exp, torch.relu = tap_exp, tap_relu
        return self.d

    def __exit__(self, *exc):
        torch.exp, torch.relu = self.exp, self.relu


def loss_and_grads(g, o, d, gt, bg, lambda_beta, lambda_sparsity, dtype):
    """(MSE part of the loss, d loss / d density_data, d loss / d sh_data) as numpy in ``dtype``"""
    g.opt.step_size, g.opt.near_clip = 0.5, 0.0
    g.density_data.grad = None
    g.sh_data.grad = None
    torch.set_default_dtype(dtype)
    try:
        with Taps() as taps:
            g.opt.background_brightness = Brightness(bg, taps)
            rays = svox2.Rays(torch.from_numpy(o).to(dtype), torch.from_numpy(d).to(dtype))
            rgb = g._volume_render_gradcheck_lerp(rays)
        mse = ((rgb - torch.from_numpy(gt).to(dtype)) ** 2).mean()
        loss = mse
        if lambda_beta:
            log_t = taps["log_t"]
            assert log_t.shape == (o.shape[0],)
            loss = loss + (lambda_beta / o.shape[0]) * (log_t + torch.log(1.0 - torch.exp(log_t) + 1e-3)).sum()
        if lambda_sparsity:
            loss = loss + lambda_sparsity * sum(torch.log(1.0 + 2.0 * s * s).sum() for s in taps["relu"])
        loss.backward()
    finally:
        torch.set_default_dtype(torch.float32)
        g.opt.background_brightness = bg
    return mse.item(), g.density_data.grad.numpy().copy(), g.sh_data.grad.numpy().copy()


def main():
    z = np.load(os.path.join(HERE, "grid_render.npz"))
    t = np.load(os.path.join(HERE, "grid_train.npz"))
    out = {}
    # ---- (a) ----
    for name in ("a", "b", "c", "d"):
        o, d, gt = z[f"{name}_origins"], z[f"{name}_dirs"], t[f"{name}_rgb_gt"]
        lb, ls = WEIGHTS[name]
        out[f"{name}_weights"] = np.array([lb, ls], dtype=np.float64)
        for tag, bg in (("bg1", 1.0), ("bg0", 0.0)):
            _, off_d, off_s = loss_and_grads(MT.grid_for(z, name, torch.float64), o, d, gt, bg, 0.0, 0.0, torch.float64)
            assert np.array_equal(off_d.astype(np.float32), t[f"{name}_{tag}_grad_density64"])      # the taps change nothing
            assert np.array_equal(off_s.astype(np.float32), t[f"{name}_{tag}_grad_sh64"])
            for setting, on_b, on_s in SETTINGS:
                args = (o, d, gt, bg, lb * on_b, ls * on_s)
                _, gd32, gs32 = loss_and_grads(MT.grid_for(z, name, torch.float32), *args, torch.float32)
                _, gd64, gs64 = loss_and_grads(MT.grid_for(z, name, torch.float64), *args, torch.float64)
                assert gd32.dtype == np.float32 and gd64.dtype == np.float64
                assert np.isfinite(gd64).all() and np.isfinite(gd32).all()
                assert np.abs(gs64 - off_s).max() <= 1e-12 * np.abs(off_s).max()      # the colours do not see the weights
                key = f"{name}_{tag}_{setting}"
                out[f"{key}_grad_density64"] = gd64.astype(np.float32)
                for k, a32, a64 in (("density", gd32, gd64), ("sh", gs32, gs64)):
                    out[f"{key}_grad_{k}_d_ref"] = np.float64(np.abs(a32.astype(np.float64) - a64).max())
                share = float(np.linalg.norm(gd64 - off_d) / np.linalg.norm(off_d))
                out[f"{key}_share"] = np.float64(share)
                print(f"grid {name} {tag} {setting}: max |g64| {np.abs(gd64).max():.3e}, d_ref density "
                      f"{out[f'{key}_grad_density_d_ref']:.3e} sh {out[f'{key}_grad_sh_d_ref']:.3e}, share {share:.3f}")
                if setting != "both":
                    assert 0.1 <= share <= 0.9, (name, tag, setting, share)
    # ---- (b) ----
    for name in ("b", "c"):
        o, d = z[f"{name}_origins"][:MT.N_POOL], z[f"{name}_dirs"][:MT.N_POOL]
        target = z[f"{name}_bg1_rgb64"][:MT.N_POOL]
        idx = t[f"{name}_loop_idx"]
        lb, ls = WEIGHTS[name]
        res = {}
        for dtype, tagd in ((torch.float32, "32"), (torch.float64, "64")):
            npdt = np.float32 if dtype == torch.float32 else np.float64
            g = MT.grid_for(z, name, dtype, (0.5 * z[f"{name}_density"]).astype(np.float32), np.zeros_like(z[f"{name}_sh"]))
            rms_d = torch.zeros_like(g.density_data.data)
            rms_s = torch.zeros_like(g.sh_data.data)
            losses, masks = [], []
            for it in range(MT.N_ITERS):
                k = idx[it]
                loss, gd, gs = loss_and_grads(g, o[k], d[k], target[k].astype(npdt), 1.0, lb, ls, dtype)
                mask = torch.from_numpy((gd != 0).any(-1) | (gs != 0).any(-1))
                with torch.no_grad():
                    MT.rmsprop(g.density_data.data, rms_d, torch.from_numpy(gd), mask, MT.LR_SIGMA)
                    MT.rmsprop(g.sh_data.data, rms_s, torch.from_numpy(gs), mask, MT.LR_SH)
                losses.append(loss)
                masks.append(mask.numpy())
            res[tagd] = (np.array(losses, dtype=np.float64), g.density_data.data.numpy().copy(), g.sh_data.data.numpy().copy(),
                         np.stack(masks))
        l32, d32, s32, m32 = res["32"]
        l64, d64, s64, m64 = res["64"]
        out.update({f"{name}_loop_loss32": l32, f"{name}_loop_loss64": l64, f"{name}_loop_density32": d32,
                    f"{name}_loop_density64": d64, f"{name}_loop_sh32": s32, f"{name}_loop_sh64": s64,
                    f"{name}_loop_mask64": np.packbits(m64, axis=-1),
                    f"{name}_loop_params": np.array([MT.BETA, MT.EPS, MT.LR_SH, MT.LR_SIGMA])})
        dl = float(np.abs(l32 - l64).max())
        moved = float(np.abs(d64 - t[f"{name}_loop_density64"]).max())
        print(f"grid {name} loop: loss {l64[0]:.4f} -> {l64[-1]:.4f}, max |l32 - l64| {dl:.2e}, final density |32 - 64| max "
              f"{np.abs(d32 - d64).max():.2e}, sh {np.abs(s32 - s64).max():.2e}, masks equal {bool((m32 == m64).all())}, "
              f"final density vs the loop without the terms: max {moved:.2e}")
        # the fixture must test the optimisation, not noise, and the terms must have moved it
        assert dl < 1e-3 * (l64[0] - l64[-1]), (name, dl, l64[0] - l64[-1])
        assert moved > 100 * np.abs(d32 - d64).max(), (name, moved)
    path = os.path.join(HERE, "grid_train_losses.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        main()
