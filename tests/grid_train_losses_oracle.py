"""numpy fp32 restatement of include/nerf_mi355x.h, "Sparse voxel grid: training with the beta and sparsity losses": the fused
step with svox2's two regularisers folded into d_sigma, and the total-variation gradient with the edge rule. It builds on
grid_train_oracle.py: ``fused`` is its ``mse_forward`` and its ``march_colour_bwd`` with the two terms switched on (the sigma they
need is what grid_oracle.march_colour's ``shade`` hook hands over), with every operation a separate fp32 rounding in the order
the header states. Like the oracles it builds on it is slow and simple, and sums into a gradient row are taken in sample
order (the kernels' atomics take them in any order).
"""
import functools

import numpy as np

import grid_oracle as GO
import grid_train_oracle as GT

F = GO.F


def beta_factor(beta_loss, log_t_final):
    """c_beta per ray: beta_loss * (1 - T_in / ((1 - T_in) + 1e-3)), fp32, each operation rounded"""
    t_in = np.exp(np.asarray(log_t_final, F)).astype(F)
    return (F(beta_loss) * (F(1.0) - (t_in / ((F(1.0) - t_in).astype(F) + F(1e-3)).astype(F)).astype(F)).astype(F)).astype(F)


def fused(grid, origins, dirs, rgb_gt, beta_loss=0.0, sparsity_loss=0.0, step_size=0.5, sigma_thresh=1e-10, stop_thresh=1e-7,
          background_brightness=1.0, near_clip=0.0, skip=None, grad_density=None, grad_sh=None, mask=None):
    """nerf_grid_fused_backward_losses: (rgb_out, grad_density, grad_sh, mask, log_transmit). ``beta_loss`` is what the kernel
    receives (lambda_beta / n_rays); T_in is this march's own final log_transmit."""
    gd, gs, mk = GT.grad_tables(grid, grad_density, grad_sh, mask)
    march = dict(step_size=step_size, sigma_thresh=sigma_thresh, stop_thresh=stop_thresh, near_clip=near_clip, skip=skip)
    rgb, log_t, gc, remaining, (Y, delta_scale, _) = GT.mse_forward(grid, origins, dirs, rgb_gt, background_brightness, **march)
    if rgb.shape[0] == 0:
        return rgb, gd, gs, mk, log_t
    shade = functools.partial(GT.march_colour_bwd, gc=gc, remaining=remaining, Y=Y, step_ds=(F(step_size) * delta_scale).astype(F),
                              grad_density=gd, grad_sh=gs, mask=mk, sparsity_loss=sparsity_loss,
                              c_beta=beta_factor(beta_loss, log_t) if beta_loss > 0 else None)
    GO.march_colour(grid, origins, dirs, shade=shade, **march)
    return rgb, gd, gs, mk, log_t


def loss_terms_density(grid, origins, dirs, beta_loss, sparsity_loss, log_transmit, step_size=0.5, sigma_thresh=1e-10,
                       stop_thresh=1e-7, near_clip=0.0, skip=None):
    """What the two terms alone add to grad_density, summed in fp64 from the fp32 factors: per shaded sample and kept corner
    w8 * (-(step_size * delta_scale) * c_beta + sparsity_factor). [capacity, 1] float64."""
    cap = grid["density_data"].shape[0]
    out = np.zeros((cap, 1), dtype=np.float64)
    _, delta_scale = GO.view_bases(grid, origins, dirs, near_clip)
    step_ds = (F(step_size) * delta_scale).astype(F)
    c_beta = beta_factor(beta_loss, log_transmit) if beta_loss > 0 else np.zeros(len(delta_scale), F)

    def shade(rays, lk, wa, wb, sigma, raw, weight, log_t_after):
        term = -step_ds[rays].astype(np.float64) * c_beta[rays].astype(np.float64)
        if sparsity_loss > 0:
            term = term + GT.sparsity_factor(sparsity_loss, sigma).astype(np.float64)
        for c, w8 in GO.corner_weights(wa, wb):
            kept = (lk[c] >= 0) & (lk[c] < cap)
            np.add.at(out[:, 0], lk[c][kept], (w8.astype(np.float64) * term)[kept])

    GO.march_colour(grid, origins, dirs, step_size, sigma_thresh, stop_thresh, near_clip, skip, shade=shade)
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
