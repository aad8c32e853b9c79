"""numpy fp32 restatement of sparse-voxel-grid training (include/nerf_mi355x.h, "Sparse voxel grid: training"): the fused
render + MSE backward with its touched-row mask, the total-variation gradient and the masked RMSProp / SGD step, with every
operation a separate fp32 rounding in the order the header states (and, as there, the one fp64 quantity of the backward:
what is still to come of a ray's colour). It builds on grid_oracle.py (same grid dict): both marches of ``fused`` are its
``march_colour``, the second with ``march_colour_bwd`` - the one backward sample, also under grid_autograd_oracle.py and
grid_train_losses_oracle.py - as the ``shade`` hook. Like it, it is a test oracle: slow and simple. Sums into a gradient row are taken in sample order (the kernels' atomics take them
in any order), so gradients agree with the kernels to rounding of those sums; the optimiser is elementwise and agrees bit
for bit.
"""
import numpy as np

import grid_oracle as GO

F = GO.F


def grad_tables(grid, grad_density=None, grad_sh=None, mask=None):
    """grad_density [C, 1], grad_sh [C, 3 B], mask [C] uint8: those passed in (they are added to), zeros otherwise"""
    cap, cols = grid["density_data"].shape[0], grid["sh_data"].shape[1]
    return (np.zeros((cap, 1), dtype=F) if grad_density is None else grad_density,
            np.zeros((cap, cols), dtype=F) if grad_sh is None else grad_sh,
            np.zeros(cap, dtype=np.uint8) if mask is None else mask)


def sparsity_factor(sparsity_loss, sigma):
    """sparsity_loss * ((4 sigma) / (1 + 2 (sigma sigma))), fp32, each operation rounded"""
    s2 = (sigma * sigma).astype(F)
    return (F(sparsity_loss) * ((F(4.0) * sigma).astype(F) / (F(1.0) + (F(2.0) * s2).astype(F)).astype(F)).astype(F)).astype(F)


def march_colour_bwd(rays, lk, wa, wb, sigma, raw, weight, log_t_after, *, gc, remaining, Y, step_ds, grad_density, grad_sh,
                     mask, c_beta=None, sparsity_loss=0.0):
    """march_colour_bwd of csrc/grid_device.h: the backward of the shaded samples of one pass, a ``shade`` hook of
    grid_oracle.march_colour once the keywords are bound. ``gc`` [N, 3] is the cotangent of rgb, ``remaining`` [N, 3] fp64
    what the samples not yet passed and the background still add to each channel (reduced here by the exact products), ``Y``
    and ``step_ds = step_size * delta_scale`` the rays' own. Adds to ``grad_density`` and ``grad_sh`` and sets ``mask``. The two
    loss terms are evaluated only when asked for: ``c_beta`` [N] (grid_train_losses_oracle.beta_factor) and ``sparsity_loss``."""
    col = np.maximum(raw, F(0.0))
    g = gc[rays]
    dot = (((col[:, 0] * g[:, 0]).astype(F) + (col[:, 1] * g[:, 1]).astype(F)).astype(F) + (col[:, 2] * g[:, 2]).astype(F)).astype(F)
    remaining[rays] -= weight[:, None].astype(np.float64) * col.astype(np.float64)
    accum = (remaining[rays] * g.astype(np.float64)).sum(-1).astype(F)
    if c_beta is not None:
        accum = (accum + c_beta[rays]).astype(F)
    d_sigma = (step_ds[rays] * ((np.exp(log_t_after).astype(F) * dot).astype(F) - accum).astype(F)).astype(F)
    if sparsity_loss > 0:
        d_sigma = (d_sigma + sparsity_factor(sparsity_loss, sigma)).astype(F)
    wy = (weight[:, None] * Y[rays]).astype(F)                                   # [n, B]
    d_coef = np.where(raw[:, :, None] >= 0, (wy[:, None, :] * g[:, :, None]).astype(F), F(0.0)).astype(F).reshape(len(rays), -1)
    for c, w8 in GO.corner_weights(wa, wb):
        kept = (lk[c] >= 0) & (lk[c] < mask.shape[0])
        rows = lk[c][kept]
        np.add.at(grad_density[:, 0], rows, (w8 * d_sigma).astype(F)[kept])
        np.add.at(grad_sh, rows, (w8[:, None] * d_coef).astype(F)[kept])
        mask[rows] = 1


def mse_forward(grid, origins, dirs, rgb_gt, background_brightness, **march):
    """The first march of a fused step: rgb_out [N, 3] with the background term, log_transmit, the cotangent ``gc`` of
    ``mean((rgb_out - rgb_gt) ** 2)``, the fp64 ``remaining`` before the first sample, and (Y, delta_scale, marched)."""
    rgb, log_t, (Y, delta_scale, marched, remaining), _ = GO.march_colour(grid, origins, dirs, **march)
    rgb = (rgb + (np.exp(log_t).astype(F) * F(background_brightness))[:, None]).astype(F)
    # what the samples not yet passed and the background still add to each channel: fp64, reduced by the exact products
    remaining += (np.exp(log_t).astype(F).astype(np.float64) * np.float64(F(background_brightness)))[:, None]
    n = rgb.shape[0]
    gc = ((rgb - np.asarray(rgb_gt, F)).astype(F) * (F(2.0) / (F(3.0) * F(n)))).astype(F) if n else rgb
    return rgb, log_t, gc, remaining, (Y, delta_scale, marched)


def fused(grid, origins, dirs, rgb_gt, step_size=0.5, sigma_thresh=1e-10, stop_thresh=1e-7, background_brightness=1.0,
          near_clip=0.0, skip=None, grad_density=None, grad_sh=None, mask=None, stats=None):
    """rgb_out [N, 3], grad_density [C, 1], grad_sh [C, 3 B], mask [C] uint8 of ``mean((rgb_out - rgb_gt) ** 2)``; the
    last three are added to when passed in. ``stats``: a dict that receives ``shaded`` (samples with sigma > sigma_thresh),
    ``clamped`` (those of them with a raw colour channel below 0) and ``marched`` (rays that were marched)."""
    gd, gs, mk = grad_tables(grid, grad_density, grad_sh, mask)
    march = dict(step_size=step_size, sigma_thresh=sigma_thresh, stop_thresh=stop_thresh, near_clip=near_clip, skip=skip)
    rgb, _, gc, remaining, (Y, delta_scale, marched) = mse_forward(grid, origins, dirs, rgb_gt, background_brightness, **march)
    if rgb.shape[0] == 0:
        return rgb, gd, gs, mk
    if stats is not None:
        stats.update(shaded=0, clamped=0, marched=int(marched.sum()))

    def shade(rays, lk, wa, wb, sigma, raw, *rest):
        if stats is not None:
            stats["shaded"] += len(rays)
            stats["clamped"] += int((raw < 0).any(-1).sum())
        march_colour_bwd(rays, lk, wa, wb, sigma, raw, *rest, gc=gc, remaining=remaining, Y=Y,
                         step_ds=(F(step_size) * delta_scale).astype(F), grad_density=gd, grad_sh=gs, mask=mk)

    GO.march_colour(grid, origins, dirs, shade=shade, **march)
    return rgb, gd, gs, mk


def tv_grad(grid, target, start, count, scale, grad, mask, start_dim=0, end_dim=None):
    """adds to ``grad`` (shaped like the table) and sets ``mask``; ``scale`` is what the kernel receives"""
    links = grid["links"]
    data = grid["density_data"] if target == "density" else grid["sh_data"]
    cap, cols = data.shape
    end_dim = cols if end_dim is None else end_dim
    X, Y, Z = links.shape
    cells = (start + np.arange(count, dtype=np.int64)) % (X * Y * Z)
    z, y, x = cells % Z, (cells // Z) % Y, cells // (Y * Z)

    def link_at(xx, yy, zz):
        inside = (xx < X) & (yy < Y) & (zz < Z)
        v = np.full(cells.shape, -1, dtype=np.int64)
        v[inside] = links[xx[inside], yy[inside], zz[inside]]
        v[(v < 0) | (v >= cap)] = -1
        return v

    lk = [link_at(x, y, z), link_at(x + 1, y, z), link_at(x, y + 1, z), link_at(x, y, z + 1)]
    sl = slice(start_dim, end_dim)
    v = [np.where((k >= 0)[:, None], data[np.maximum(k, 0)][:, sl], F(0.0)).astype(F) for k in lk]
    dx, dy, dz = (v[1] - v[0]).astype(F), (v[2] - v[0]).astype(F), (v[3] - v[0]).astype(F)
    ss = (((F(1e-9) + (dx * dx).astype(F)).astype(F) + (dy * dy).astype(F)).astype(F) + (dz * dz).astype(F)).astype(F)
    idelta = (F(scale) / np.sqrt(ss).astype(F)).astype(F)
    dx = (dx * (F(X) * F(1.0 / 256.0))).astype(F)
    dy = (dy * (F(Y) * F(1.0 / 256.0))).astype(F)
    dz = (dz * (F(Z) * F(1.0 / 256.0))).astype(F)
    vals = [(-((dx + dy).astype(F) + dz).astype(F)).astype(F), dx, dy, dz]
    for k, val in zip(lk, vals):
        add = (val * idelta).astype(F)
        use = (k >= 0)[:, None] & (val != 0)
        r, c = np.nonzero(use)
        np.add.at(grad, (k[r], c + start_dim), add[r, c])
        mask[k[r]] = 1


def optim_step(data, rms, grad, mask, kind, lr, beta=0.95, eps=1e-8, minval=-1e9):
    """in place on the rows with mask != 0 (any non-zero byte); ``kind`` "rmsprop" or "sgd"; every operation one IEEE fp32
    rounding, subnormals kept. ``max`` is C ``fmaxf`` (np.fmax): a NaN operand is dropped, so an element whose update is NaN
    lands on ``minval`` (np.maximum would keep the NaN). A NaN in ``rms`` stays there."""
    m = np.asarray(mask) != 0
    g = grad[m].astype(F)
    with np.errstate(all="ignore"):      # non-finite and subnormal inputs are ordinary inputs here
        if kind == "rmsprop":
            g2 = (g * g).astype(F)
            r = rms[m]
            r = np.where(r == 0, g2, (g2 + (F(beta) * (r - g2).astype(F)).astype(F)).astype(F)).astype(F)
            rms[m] = r
            upd = ((F(lr) * g).astype(F) / (np.sqrt(r).astype(F) + F(eps)).astype(F)).astype(F)
        else:
            upd = (F(lr) * g).astype(F)
        data[m] = np.fmax((data[m] - upd).astype(F), F(minval)).astype(F)
