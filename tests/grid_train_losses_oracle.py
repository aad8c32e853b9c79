"""numpy fp32 restatement of include/nerf_mi355x.h, "Sparse voxel grid: training with the beta and sparsity losses": the fused
step with svox2's two regularisers folded into d_sigma, and the total-variation gradient with the edge rule. It builds on
grid_train_oracle._march and its ``shade`` hook (the hook does not hand over sigma: it is interpolated again from the links and
weights it does hand over, the same operations on the same values), with every operation a separate fp32 rounding in the
order the header states. Like the oracles it builds on it is slow and simple, and sums into a gradient row are taken in
sample order (the kernels' atomics take them in any order).
"""
import numpy as np

import grid_oracle as GO
import grid_train_oracle as GT

F = GO.F


def beta_factor(beta_loss, log_t_final):
    """c_beta per ray: beta_loss * (1 - T_in / ((1 - T_in) + 1e-3)), fp32, each operation rounded"""
    t_in = np.exp(np.asarray(log_t_final, F)).astype(F)
    return (F(beta_loss) * (F(1.0) - (t_in / ((F(1.0) - t_in).astype(F) + F(1e-3)).astype(F)).astype(F)).astype(F)).astype(F)


def sparsity_factor(sparsity_loss, sigma):
    """sparsity_loss * ((4 sigma) / (1 + 2 (sigma sigma))), fp32, each operation rounded"""
    s2 = (sigma * sigma).astype(F)
    return (F(sparsity_loss) * ((F(4.0) * sigma).astype(F) / (F(1.0) + (F(2.0) * s2).astype(F)).astype(F)).astype(F)).astype(F)


def _sigma(grid, lk, wa, wb):
    return GO._trilerp([GO._fetch(grid, k, grid["density_data"]) for k in lk], wa, wb)[:, 0]


def _corner_weights(wa, wb):
    for c in range(8):
        wx = wb[:, 0] if c & 4 else wa[:, 0]
        wy = wb[:, 1] if c & 2 else wa[:, 1]
        wz = wb[:, 2] if c & 1 else wa[:, 2]
        yield c, ((wx * wy).astype(F) * wz).astype(F)


def fused(grid, origins, dirs, rgb_gt, beta_loss=0.0, sparsity_loss=0.0, step_size=0.5, sigma_thresh=1e-10, stop_thresh=1e-7,
          background_brightness=1.0, near_clip=0.0, skip=None, grad_density=None, grad_sh=None, mask=None):
    """nerf_grid_fused_backward_losses: (rgb_out, grad_density, grad_sh, mask, log_transmit). ``beta_loss`` is what the kernel
    receives (lambda_beta / n_rays); T_in is this march's own final log_transmit."""
    cap, cols = grid["density_data"].shape[0], grid["sh_data"].shape[1]
    B = cols // 3
    gd = np.zeros((cap, 1), dtype=F) if grad_density is None else grad_density
    gs = np.zeros((cap, cols), dtype=F) if grad_sh is None else grad_sh
    mk = np.zeros(cap, dtype=np.uint8) if mask is None else mask
    args = (grid, origins, dirs, step_size, sigma_thresh, stop_thresh, near_clip, skip)
    rgb, log_t, (Y, delta_scale, marched, remaining) = GT._march(*args)
    rgb = (rgb + (np.exp(log_t).astype(F) * F(background_brightness))[:, None]).astype(F)
    remaining += (np.exp(log_t).astype(F).astype(np.float64) * np.float64(F(background_brightness)))[:, None]
    n = rgb.shape[0]
    if n == 0:
        return rgb, gd, gs, mk, log_t
    scale = F(2.0) / (F(3.0) * F(n))
    gc = ((rgb - np.asarray(rgb_gt, F)).astype(F) * scale).astype(F)
    step_ds = (F(step_size) * delta_scale).astype(F)
    c_beta = beta_factor(beta_loss, log_t)

    def shade(rays, lk, wa, wb, raw, weight, log_t_after):
        col = np.maximum(raw, F(0.0))
        g = gc[rays]
        dot = (((col[:, 0] * g[:, 0]).astype(F) + (col[:, 1] * g[:, 1]).astype(F)).astype(F) + (col[:, 2] * g[:, 2]).astype(F)).astype(F)
        remaining[rays] -= weight[:, None].astype(np.float64) * col.astype(np.float64)
        accum = (remaining[rays] * g.astype(np.float64)).sum(-1).astype(F)
        if beta_loss > 0:
            accum = (accum + c_beta[rays]).astype(F)
        d_sigma = (step_ds[rays] * ((np.exp(log_t_after).astype(F) * dot).astype(F) - accum).astype(F)).astype(F)
        if sparsity_loss > 0:
            d_sigma = (d_sigma + sparsity_factor(sparsity_loss, _sigma(grid, lk, wa, wb))).astype(F)
        wy = (weight[:, None] * Y[rays]).astype(F)
        d_coef = np.where(raw[:, :, None] >= 0, (wy[:, None, :] * g[:, :, None]).astype(F), F(0.0)).astype(F).reshape(-1, 3 * B)
        for c, w8 in _corner_weights(wa, wb):
            kept = (lk[c] >= 0) & (lk[c] < cap)
            rows = lk[c][kept]
            np.add.at(gd[:, 0], rows, (w8 * d_sigma).astype(F)[kept])
            np.add.at(gs, rows, (w8[:, None] * d_coef).astype(F)[kept])
            mk[rows] = 1

    GT._march(*args, shade=shade)
    return rgb, gd, gs, mk, log_t


def loss_terms_density(grid, origins, dirs, beta_loss, sparsity_loss, log_transmit, step_size=0.5, sigma_thresh=1e-10,
                       stop_thresh=1e-7, near_clip=0.0, skip=None):
    """What the two terms alone add to grad_density, summed in fp64 from the fp32 factors: per shaded sample and kept corner
    w8 * (-(step_size * delta_scale) * c_beta + sparsity_factor). [capacity, 1] float64."""
    cap = grid["density_data"].shape[0]
    out = np.zeros((cap, 1), dtype=np.float64)
    args = (grid, origins, dirs, step_size, sigma_thresh, stop_thresh, near_clip, skip)
    _, _, (_, delta_scale, _, _) = GT._march(*args)
    step_ds = (F(step_size) * delta_scale).astype(F)
    c_beta = beta_factor(beta_loss, log_transmit) if beta_loss > 0 else np.zeros(len(delta_scale), F)

    def shade(rays, lk, wa, wb, raw, weight, log_t_after):
        term = -step_ds[rays].astype(np.float64) * c_beta[rays].astype(np.float64)
        if sparsity_loss > 0:
            term = term + sparsity_factor(sparsity_loss, _sigma(grid, lk, wa, wb)).astype(np.float64)
        for c, w8 in _corner_weights(wa, wb):
            kept = (lk[c] >= 0) & (lk[c] < cap)
            np.add.at(out[:, 0], lk[c][kept], (w8.astype(np.float64) * term)[kept])

    GT._march(*args, shade=shade)
    return out


def tv_grad(grid, target, start, count, scale, grad, mask, start_dim=0, end_dim=None, ignore_edge=True):
    """nerf_grid_tv_grad_edge: adds to ``grad`` (shaped like the table) and sets ``mask``; ``scale`` is what the kernel
    receives. With ``ignore_edge`` false it is grid_train_oracle.tv_grad."""
    if not ignore_edge:
        return GT.tv_grad(grid, target, start, count, scale, grad, mask, start_dim, end_dim)
    links = grid["links"]
    data = grid["density_data"] if target == "density" else grid["sh_data"]
    cap, cols = data.shape
    end_dim = cols if end_dim is None else end_dim
    X, Y, Z = links.shape
    cells = (start + np.arange(count, dtype=np.int64)) % (X * Y * Z)
    z, y, x = cells % Z, (cells // Z) % Y, cells // (Y * Z)
    cells = cells[links[x, y, z] != 0]      # the reference's literal test: the cell whose own link is row 0 does nothing
    z, y, x = cells % Z, (cells // Z) % Y, cells // (Y * Z)

    def link_at(xx, yy, zz):
        inside = (xx < X) & (yy < Y) & (zz < Z)
        v = np.full(cells.shape, -1, dtype=np.int64)
        v[inside] = links[xx[inside], yy[inside], zz[inside]]
        v[(v < 0) | (v >= cap)] = -1
        return v

    lk = [link_at(x, y, z), link_at(x + 1, y, z), link_at(x, y + 1, z), link_at(x, y, z + 1)]
    sl = slice(start_dim, end_dim)
    v0 = np.where((lk[0] >= 0)[:, None], data[np.maximum(lk[0], 0)][:, sl], F(0.0)).astype(F)
    v = [v0] + [np.where((k >= 0)[:, None], data[np.maximum(k, 0)][:, sl], v0).astype(F) for k in lk[1:]]
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
