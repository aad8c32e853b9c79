#!/usr/bin/env python3
"""Generate tests/golden/train_autograd.npz from the REFERENCE itself: loss.backward() of a loss on every differentiable
output of render_rays (tests/autograd_losses.py) through the reference's own autograd.

Like make_golden.py (whose helpers it imports) it runs only where the reference checkout is present; the fixture holds
arrays only. The batch is the 32 rays of train_step.npz with gold_train's kwargs (64 + 128 samples, white_bkgd, perturb,
sigma noise, the reference's pytest RNG, retraw) plus two constructed rays at raw2outputs' kinks:
- an EMPTY ray (acc = 0): its samples all sit at one point of negative density. max(1e-10, acc) and clamp(min=1e-10) both
  take their other side, and the gradient must come out as zeros, not NaN. (In fp32 this is the only way below the max's
  kink: 1 - exp(-x) is 0 or at least 2^-24, so acc < 1e-10 means acc = 0, depth = 0, and the clamp then stops the gradient
  before it reaches the max.)
- a SHALLOW ray: depths in [0, 1e-11] at a point of positive density, with a long direction so that the samples' opacities
  are moderate. Its acc is of order 1 but depth / acc < 1e-10, so clamp(min=1e-10) stops a nonzero dL/d disp. The
  generator checks that a clamp passing the gradient instead would change the gradients far beyond the test's bars.
The reference runs once in fp32 and once in fp64; stored for both: the fine depths, the loss value, and per-tensor
gradient norms plus every 61st element (as gold_train stores them).

    python tests/golden/make_golden_autograd.py        # rewrites tests/golden/train_autograd.npz
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402  (reference helpers; needs the reference checkout)
from autograd_losses import autograd_loss  # noqa: E402


def constructed_rays(net_c, net_f):
    """The empty ray: origin at the first point of a seeded search at which both networks' sigma is below -1.2 (the pytest
    noise is uniform in [0, 1)), direction 1e-12 long (every sample at the origin). The shallow ray: origin at the first
    point where both are above 2, depths [0, 1e-11], direction 3e10 long (per-sample optical depths of a few hundredths)."""
    e_fn, _ = mg.ref_embedder.get_embedder(10, 0)
    ed_fn, _ = mg.ref_embedder.get_embedder(4, 0)
    q = mg.query_fn(e_fn, ed_fn)
    pts = torch.from_numpy(np.random.RandomState(5).uniform(-6, 6, size=(4096, 1, 3)).astype(np.float32))
    vd = torch.from_numpy(np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (4096, 1)))
    with torch.no_grad():
        sc, sf = q(pts, vd, net_c)[:, 0, 3].numpy(), q(pts, vd, net_f)[:, 0, 3].numpy()
    i = int(np.where((sc < -1.2) & (sf < -1.2))[0][0])
    j = int(np.where((sc > 2.0) & (sf > 2.0))[0][0])
    empty = np.concatenate([pts[i, 0].numpy(), [0.0, 0.0, 1e-12], [2.0, 6.0], [0.0, 0.0, 1.0]])
    shallow = np.concatenate([pts[j, 0].numpy(), [0.0, 0.0, 3e10], [0.0, 1e-11], [0.0, 0.0, 1.0]])
    return np.stack([empty, shallow]).astype(np.float32)


class _PassingClamp:
    """torch with a clamp that passes the gradient everywhere: the wrong convention, to show the fixture tells them apart"""
    def __getattr__(self, k):
        return getattr(torch, k)

    @staticmethod
    def clamp(x, min=None, max=None):
        return x + (torch.clamp(x, min=min, max=max) - x).detach()


def run(rays, target, dtype, wrong_clamp=False):
    net_c, net_f = mg.ref_pair(0, dtype)
    net_c.train(); net_f.train()
    e_fn, _ = mg.ref_embedder.get_embedder(10, 0)
    ed_fn, _ = mg.ref_embedder.get_embedder(4, 0)
    z_fine = []
    orig = mg.NS["raw2outputs"]

    def r2o(raw, z_vals, *a, **k):
        z_fine.append(mg.n(z_vals))
        return orig(raw, z_vals, *a, **k)

    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    mg.NS["raw2outputs"] = r2o
    if wrong_clamp:
        mg.NS["torch"] = _PassingClamp()
    try:
        ret = mg.NS["render_rays"](torch.from_numpy(rays).to(dtype), net_c, mg.query_fn(e_fn, ed_fn), network_fine=net_f,
                                   N_samples=64, N_importance=128, retraw=True, white_bkgd=True, perturb=1.0,
                                   raw_noise_std=1.0, pytest=True)
        loss = autograd_loss(ret, torch.from_numpy(target).to(dtype))
        loss.backward()
    finally:
        mg.NS["raw2outputs"] = orig
        mg.NS["torch"] = torch
        torch.set_default_dtype(old)
    out = {"loss": mg.n(loss), "z_fine": z_fine[1], "acc": mg.n(ret["acc_map"]), "acc0": mg.n(ret["acc0"]),
           "disp": mg.n(ret["disp_map"]), "disp0": mg.n(ret["disp0"])}
    for tag, net in (("c", net_c), ("f", net_f)):
        for k, p in net.named_parameters():
            gr = mg.n(p.grad).reshape(-1) if p.grad is not None else np.zeros(p.numel(), mg.n(p).dtype)
            out[f"gnorm_{tag}.{k}"] = np.linalg.norm(gr.astype(np.float64))
            out[f"gsub_{tag}.{k}"] = gr[::61].copy()
    return out


def main():
    g = np.load(os.path.join(HERE, "train_step.npz"))
    net_c, net_f = mg.ref_pair(0)
    rays = np.concatenate([g["rays"], constructed_rays(net_c, net_f)], 0)
    target = np.concatenate([g["target"], np.random.RandomState(107).uniform(0, 1, size=(2, 3)).astype(np.float32)], 0)
    out = dict(rays=rays, target=target)
    for name, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        for k, v in run(rays, target, dtype).items():
            out[f"{name}.{k}"] = v
    for p in ("", "0"):
        acc, disp = out[f"f32.acc{p}"], out[f"f32.disp{p}"]
        assert acc[-2] == 0.0 and disp[-2] > 1e9, "the empty ray is not empty"
        assert acc[-1] > 0.05 and disp[-1] > 1e9, ("the shallow ray is not at the clamp", acc[-1], disp[-1])
    # the shallow ray tells the conventions apart: a clamp that passes the gradient moves the gradients by far more than
    # the test's bars (2e-5 / 1e-4 of a tensor's largest element)
    wrong = run(rays, target, torch.float32, wrong_clamp=True)
    moved = max(np.abs(wrong[k] - out["f32." + k]).max() / (np.abs(out["f64." + k]).max() + 1e-30)
                for k in wrong if k.startswith("gsub_"))
    print("a passing clamp moves the gradients by %.3g of a tensor's largest element" % moved)
    assert moved > 1e-2, moved
    print("loss f32 %.9g f64 %.17g" % (out["f32.loss"], out["f64.loss"]))
    mg.save("train_autograd", **out)


if __name__ == "__main__":
    main()
