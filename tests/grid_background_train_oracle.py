"""numpy restatement of training the background layers (include/nerf_mi355x.h, "Sparse voxel grid: background layers,
training"): the taped background pass, its backward, the total-variation gradient of the layers and their optimiser step, in
the dtype ``T`` - ``np.float32`` with every operation a separate rounding in the order the header states (the kernels'
arithmetic; ``remaining`` in fp64 as there), or ``np.float64`` (the same formulas, exact enough to compare with fp64
autograd). It builds on grid_background_oracle.py (the stages and ``march``, the one loop over the spheres: the taped
pass and the backward are its ``shade`` hooks), on grid_autograd_oracle.py (the foreground: ``render_taped``, ``render_backward``)
and on grid_train_oracle.py (``optim_step``) and, like them, is a test oracle: slow and simple. Sums into a gradient entry are taken in step order (the kernels' atomics take
them in any order), so gradients agree with the kernels to rounding of those sums; the optimiser agrees bit for bit.
A background is a dict: ``links`` int32 [2 R, R], ``data`` fp32 [capacity, L, 4].
"""
import numpy as np

import grid_autograd_oracle as GA
import grid_background_oracle as BO
import grid_oracle as GO
import grid_train_oracle as GT

F = np.float32
D = np.float64
SH_C0 = BO.SH_C0


def taped(o, d, delta_scale, ok, reso, bg, rgb, log_transmit, tape, step_size=0.5, stop_thresh=1e-7, background_brightness=1.0,
          T=F, return_stats=False):
    """nerf_grid_background_rays_taped: (rgb [n, 3] in ``T``, log_transmit_out [n] in ``T``, tape [n, 3] fp64, tape_background
    [n, 3] fp64) from the foreground's ``rgb``, ``log_transmit`` (converted to ``T``) and ``tape``."""
    rgb_in, log_in = np.asarray(rgb).astype(T), np.asarray(log_transmit).astype(T)
    n = rgb_in.shape[0]
    out = np.zeros((n, 3), T)
    tot = np.zeros((n, 3), D)
    R = bg["links"].shape[1]
    seen = dict(seam_x=np.zeros(n, bool), seam_y=np.zeros(n, bool), clamped=np.zeros(n, bool))

    def shade(idx, l, w, v, dstep, weight, log_t):
        with np.errstate(invalid="ignore"):
            raw = ((v[:, :3] * T(SH_C0)).astype(T) + T(0.5)).astype(T)
            col = np.maximum(raw, T(0.0)).astype(T)
        out[idx] = (out[idx] + (weight[:, None] * col).astype(T)).astype(T)
        tot[idx] += weight[:, None].astype(D) * col.astype(D)
        seen["seam_x"][idx] |= l[:, 0] == 2 * R - 1
        seen["seam_y"][idx] |= l[:, 1] == R - 1
        seen["clamped"][idx] |= (raw < 0).any(-1)

    run, left_alone, log_t, stats = BO.march(o, d, delta_scale, ok, reso, bg, log_in, step_size, stop_thresh, T, shade)
    bright = T(F(background_brightness))
    with np.errstate(all="ignore"):
        e_end, e_in = np.exp(log_t).astype(T), np.exp(log_in).astype(T)
        full = rgb_in + (out + (e_end * bright)[:, None])
        only = rgb_in + (e_in * bright)[:, None]
    only_rays = ~left_alone & ~run
    rgb_out = np.where(run[:, None], full, np.where(only_rays[:, None], only, rgb_in)).astype(T)
    log_out = np.where(run, log_t, log_in).astype(T)
    tb = np.where(run[:, None], tot + (e_end.astype(D) * D(bright))[:, None],
                  np.where(only_rays[:, None], (e_in.astype(D) * D(bright))[:, None], 0.0))
    tape_out = np.asarray(tape, D) + tb
    if return_stats:
        stats.update(seen, left_alone=left_alone, run=run)
        return rgb_out, log_out, tape_out, tb, stats
    return rgb_out, log_out, tape_out, tb


def backward(o, d, delta_scale, ok, reso, bg, grad_rgb, log_transmit, tape_background, step_size=0.5, stop_thresh=1e-7,
             grad=None, mask=None, T=F):
    """nerf_grid_background_backward: adds to ``grad`` [capacity, L, 4] (dtype ``T``) and sets ``mask`` [capacity, L] uint8;
    both are made when not passed in. ``log_transmit`` is the foreground's."""
    links, data = bg["links"], bg["data"]
    cap, L = data.shape[0], data.shape[1]
    R2, R = links.shape
    flat = links.reshape(-1)
    gb = np.zeros((cap, L, 4), T) if grad is None else grad
    mk = np.zeros((cap, L), np.uint8) if mask is None else mask
    g_all = np.asarray(grad_rgb).astype(T)
    remaining = np.array(tape_background, D)
    log_in = np.asarray(log_transmit).astype(T)

    def shade(idx, l, w, v, dstep, weight, log_t):
        g = g_all[idx]
        col = ((v[:, :3] * T(SH_C0)).astype(T) + T(0.5)).astype(T)
        cc = np.maximum(col, T(0.0))
        dot = (((cc[:, 0] * g[:, 0]).astype(T) + (cc[:, 1] * g[:, 1]).astype(T)).astype(T) + (cc[:, 2] * g[:, 2]).astype(T)).astype(T)
        remaining[idx] -= weight[:, None].astype(D) * cc.astype(D)
        accum = (remaining[idx] * g.astype(D)).sum(-1).astype(T)
        with np.errstate(all="ignore"):
            d_sigma = (dstep * ((np.exp(log_t).astype(T) * dot).astype(T) - accum).astype(T)).astype(T)
        d_col = np.where(col > 0, ((T(SH_C0) * weight).astype(T)[:, None] * g).astype(T), T(0.0)).astype(T)
        gv = np.concatenate([d_col, d_sigma[:, None]], -1).astype(T)      # [m, 4]
        lx, ly, lz = l[:, 0], l[:, 1], l[:, 2]
        nx = np.where(lx < R2 - 1, lx + 1, 0)
        ny = np.where(ly < R - 1, ly + 1, 0)
        wx, wy, wz = w[:, 0], w[:, 1], w[:, 2]
        one = T(1.0)
        for X, fx in ((lx, (one - wx).astype(T)), (nx, wx)):
            xo = (fx[:, None] * gv).astype(T)
            for Y, fy in ((ly, (one - wy).astype(T)), (ny, wy)):
                val = (fy[:, None] * xo).astype(T)
                lk = flat[X * R + Y].astype(np.int64)
                has = (lk >= 0) & (lk < cap)
                for zz, fz in ((lz, (one - wz).astype(T)), (lz + 1, wz)):
                    add = (val * fz[:, None]).astype(T)
                    r, c = np.nonzero(has[:, None] & (add != 0))
                    np.add.at(gb, (lk[r], zz[r], c), add[r, c])
                    mk[lk[has], zz[has]] = 1

    BO.march(o, d, delta_scale, ok, reso, bg, log_in, step_size, stop_thresh, T, shade)
    return gb, mk


def tv_grad(bg, start, count, scale_sigma, scale_color, grad, mask, T=F):
    """nerf_grid_background_tv_grad: adds to ``grad`` [capacity, L, 4] and sets ``mask`` [capacity, L]; the scales are what
    the kernel receives."""
    links, data = bg["links"], np.asarray(bg["data"], F).astype(T)
    cap, L = data.shape[0], data.shape[1]
    R2, R = links.shape
    cells = (start + np.arange(count, dtype=np.int64)) % (R2 * R * L)
    z, y, x = cells % L, (cells // L) % R, cells // (L * R)
    nx = np.where(x < R2 - 1, x + 1, 0)
    ny = np.where(y < R - 1, y + 1, 0)

    def link_at(X, Y):
        lk = links[X, Y].astype(np.int64)
        lk[(lk < 0) | (lk >= cap)] = -1
        return lk

    l00, l10, l01 = link_at(x, y), link_at(nx, y), link_at(x, ny)
    val = lambda lk, zz: np.where((lk >= 0)[:, None], data[np.maximum(lk, 0), zz], T(0.0)).astype(T)      # noqa: E731
    v00, v10, v01 = val(l00, z), val(l10, z), val(l01, z)
    has_z = (l00 >= 0) & (z + 1 < L)
    edge = v00.copy()
    edge[:, 3] = T(0.0)
    v_nxl = np.where(has_z[:, None], data[np.maximum(l00, 0), np.minimum(z + 1, L - 1)], edge).astype(T)
    dx, dy, dz = (v10 - v00).astype(T), (v01 - v00).astype(T), (v_nxl - v00).astype(T)
    scale = np.array([scale_color, scale_color, scale_color, scale_sigma], F).astype(T)
    ss = (((T(1e-9) + (dx * dx).astype(T)).astype(T) + (dy * dy).astype(T)).astype(T) + (dz * dz).astype(T)).astype(T)
    idelta = (scale[None, :] / np.sqrt(ss).astype(T)).astype(T)
    dx = (dx * (T(R2) * T(F(1.0 / 256.0)))).astype(T)
    dy = (dy * (T(R) * T(F(1.0 / 256.0)))).astype(T)
    dz = (dz * (T(L) * T(F(1.0 / 256.0)))).astype(T)
    terms = [(l00, z, l00 >= 0, (-((dx + dy).astype(T) + dz).astype(T)).astype(T)), (l00, z + 1, has_z, dz), (l01, z, l01 >= 0, dy),
             (l10, z, l10 >= 0, dx)]
    for lk, zz, has, t in terms:
        add = (t * idelta).astype(T)
        r, c = np.nonzero(has[:, None] & (add != 0))
        np.add.at(grad, (lk[r], zz[r], c), add[r, c])
        mask[lk[r], zz[r]] = 1


def optim_step(data, rms, grad, mask, kind, lr_sigma, lr_color, beta=0.95, eps=1e-8, minval=-1e9):
    """nerf_grid_background_optim_step in place on data [capacity, L, 4]: grid_train_oracle.optim_step per column, with
    ``lr_color`` for the columns 0..2 and ``lr_sigma`` for column 3."""
    cap, L = data.shape[0], data.shape[1]
    for c in range(4):
        dc, rc = np.ascontiguousarray(data[..., c]).reshape(cap * L, 1), np.ascontiguousarray(rms[..., c]).reshape(cap * L, 1)
        GT.optim_step(dc, rc, np.ascontiguousarray(grad[..., c]).reshape(cap * L, 1), np.asarray(mask).reshape(-1), kind,
                      lr_sigma if c == 3 else lr_color, beta, eps, minval)
        data[..., c] = dc.reshape(cap, L)
        rms[..., c] = rc.reshape(cap, L)


def forward_backward(grid, bg, origins, dirs, rgb_gt, step_size=0.5, sigma_thresh=1e-10, stop_thresh=1e-7,
                     background_brightness=1.0, skip=None, grad_rgb=None, state=None):
    """BackgroundTrainer.forward_backward in fp32: the taped foreground (brightness 0), the taped background pass, the MSE
    cotangent (or ``grad_rgb``), the foreground's backward from the combined tape, the background's backward. Returns a dict:
    rgb, log_transmit, grad_density, grad_sh, mask, grad_background, mask_background (``state``: such a dict to add to)."""
    fg_rgb, fg_logt, tot = GA.render_taped(grid, origins, dirs, step_size, sigma_thresh, stop_thresh, background_brightness=0.0, skip=skip)
    og, dg, _, ds, _, _, ok = GO.ray_setup(grid, origins, dirs)
    reso = grid["links"].shape
    rgb, logt, tape, tb = taped(og, dg, ds, ok, reso, bg, fg_rgb, fg_logt, tot, step_size, stop_thresh, background_brightness)
    n = rgb.shape[0]
    if grad_rgb is None:
        grad_rgb = ((rgb - np.asarray(rgb_gt, F)).astype(F) * (F(2.0) / (F(3.0) * F(n)))).astype(F)
    st = state or {}
    gd, gs, mk = GA.render_backward(grid, origins, dirs, grad_rgb, tape, step_size, sigma_thresh, stop_thresh, 0.0, skip,
                                    st.get("grad_density"), st.get("grad_sh"), st.get("mask"))
    gb, mb = backward(og, dg, ds, ok, reso, bg, grad_rgb, fg_logt, tb, step_size, stop_thresh, st.get("grad_background"),
                      st.get("mask_background"))
    return dict(rgb=rgb, log_transmit=logt, grad_density=gd, grad_sh=gs, mask=mk, grad_background=gb, mask_background=mb,
                grad_rgb=grad_rgb, fg_log_transmit=fg_logt)
