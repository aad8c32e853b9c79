"""Writes tests/golden/grid_train_variants.npz: the reference's autograd gradients of the MSE loss off the one setting that
tests/golden/grid_train.npz records (step_size 0.5, near_clip 0, background 0 or 1).

    NERF_REFERENCE_SVOX2=/path/to/reference/svox2 python tests/golden/make_golden_grid_train_variants.py

At the recorded setting three terms of the backward vanish or are constant: ``step_size * delta_scale``, the background's
part of what is still to come of a ray's colour, and the clamp of tmin to ``near_clip``. Here they are not:

    grid a: step (background 1, step_size 0.3, near_clip 0), near (1, 0.5, 6.0), mix (0.5, 0.8, 2.5)
    grids b and c: mix

The grids, the 1024 rays and ``gt`` (``*_rgb_gt``) are those of grid_render.npz / grid_train.npz. As there, PyTorch autograd
through ``SparseGrid._volume_render_gradcheck_lerp`` (the CUDA semantics at ``sigma_thresh = 0``, ``stop_thresh = 0``), once
on fp32 and once on fp64 tensors; per case the fp64 gradients rounded to fp32, the fp64 loss and ``d_ref`` = max |fp32
gradient - fp64 gradient| per tensor. Runs on the CPU in seconds. Nothing of the reference is copied: arrays only.
"""
import os
import warnings

import numpy as np
import torch

import make_golden_grid_train as MT  # (this project's; imports svox2 from NERF_REFERENCE_SVOX2)

HERE = os.path.dirname(os.path.abspath(__file__))
svox2 = MT.svox2
# (tag, background_brightness, step_size, near_clip)
VARIANTS = {"step": (1.0, 0.3, 0.0), "near": (1.0, 0.5, 6.0), "mix": (0.5, 0.8, 2.5)}
CASES = [("a", "step"), ("a", "near"), ("a", "mix"), ("b", "mix"), ("c", "mix")]


def loss_and_grads(z, name, o, d, gt, variant, dtype):
    bg, step, near = variant
    g = MT.grid_for(z, name, dtype)
    g.opt.background_brightness, g.opt.step_size, g.opt.near_clip = bg, step, near
    torch.set_default_dtype(dtype)
    try:
        rays = svox2.Rays(torch.from_numpy(o).to(dtype), torch.from_numpy(d).to(dtype))
        rgb = g._volume_render_gradcheck_lerp(rays)
        loss = ((rgb - torch.from_numpy(gt).to(dtype)) ** 2).mean()
        loss.backward()
    finally:
        torch.set_default_dtype(torch.float32)
    return loss.item(), g.density_data.grad.numpy().copy(), g.sh_data.grad.numpy().copy()


def main():
    z = np.load(os.path.join(HERE, "grid_render.npz"))
    t = np.load(os.path.join(HERE, "grid_train.npz"))
    out = {}
    for name, tag in CASES:
        o, d, gt = z[f"{name}_origins"], z[f"{name}_dirs"], t[f"{name}_rgb_gt"]
        _, gd32, gs32 = loss_and_grads(z, name, o, d, gt, VARIANTS[tag], torch.float32)
        l64, gd64, gs64 = loss_and_grads(z, name, o, d, gt, VARIANTS[tag], torch.float64)
        assert gd32.dtype == np.float32 and gd64.dtype == np.float64
        out[f"{name}_{tag}_variant"] = np.array(VARIANTS[tag], dtype=np.float64)
        out[f"{name}_{tag}_grad_density64"] = gd64.astype(np.float32)
        out[f"{name}_{tag}_grad_sh64"] = gs64.astype(np.float32)
        out[f"{name}_{tag}_loss64"] = np.float64(l64)
        for key, a32, a64 in (("density", gd32, gd64), ("sh", gs32, gs64)):
            d_ref = float(np.abs(a32.astype(np.float64) - a64).max())
            out[f"{name}_{tag}_grad_{key}_d_ref"] = np.float64(d_ref)
            print(f"grid {name} {tag} d/d{key}: max |g64| {np.abs(a64).max():.3e}, |fp32 - fp64| max {d_ref:.3e} "
                  f"= {d_ref / np.abs(a64).max():.2e} of it, rows != 0: {int((a64 != 0).any(-1).sum())} of {a64.shape[0]}")
    path = os.path.join(HERE, "grid_train_variants.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        main()
