"""numpy fp32 restatement of sparse-voxel-grid training (include/nerf_mi355x.h, "Sparse voxel grid: training"): the fused
render + MSE backward with its touched-row mask, the total-variation gradient and the masked RMSProp / SGD step, with every
operation a separate fp32 rounding in the order the header states (and, as there, the one fp64 quantity of the backward:
what is still to come of a ray's colour). It builds on grid_oracle.py (same grid dict) and, like
it, is a test oracle: slow and simple. Sums into a gradient row are taken in sample order (the kernels' atomics take them
in any order), so gradients agree with the kernels to rounding of those sums; the optimiser is elementwise and agrees bit
for bit.
"""
import numpy as np

import grid_oracle as GO

F = GO.F


def _march(grid, origins, dirs, step_size, sigma_thresh, stop_thresh, near_clip, skip, shade=None):
    """grid_oracle.render's march. Returns (rgb without the background term, log_transmit, (..., the same colour summed in
    fp64)). ``shade(rays, lk, wa, wb, col_raw, weight, log_t_after)`` is called once per step of the march with the shaded samples of that step."""
    links, density, sh = grid["links"], grid["density_data"], grid["sh_data"]
    B = sh.shape[1] // 3
    step = F(step_size)
    o, g, view, delta_scale, tmin, tmax, ok = GO.ray_setup(grid, origins, dirs, near_clip)
    Y = GO.sh_bases(B, np.where(ok[:, None], view, F(0.0)).astype(F))
    n = o.shape[0]
    rgb = np.zeros((n, 3), dtype=F)
    tot = np.zeros((n, 3), dtype=np.float64)      # the colour once more, as the fp64 sum of its exact terms
    log_t = np.zeros(n, dtype=F)
    t = tmin.copy()
    with np.errstate(invalid="ignore"):
        skip_ok = (np.abs(o).max(-1) < GO.SKIP_MAX_T) & (np.abs(tmin) < GO.SKIP_MAX_T) & (np.abs(tmax) < GO.SKIP_MAX_T)
        marched = ok & (tmin <= tmax)
    act = np.nonzero(marched)[0]
    while act.size:
        t_next = (t[act] + step).astype(F)
        act, t_next = act[t_next > t[act]], t_next[t_next > t[act]]
        if not act.size:
            break
        pos = (o[act] + t[act, None] * g[act]).astype(F)
        l, wb = GO._cell(pos, links.shape)
        wa = (F(1.0) - wb).astype(F)
        sv = np.zeros(act.size, dtype=np.int64)
        if skip is not None:
            sv = np.where(skip_ok[act], skip[l[:, 0], l[:, 1], l[:, 2]].astype(np.int64), 0)
        work = sv == 0
        stopped = np.zeros(act.size, dtype=bool)
        if work.any():
            w_idx = np.nonzero(work)[0]
            lk = [k[w_idx] for k in GO._corner_links(links, l)]
            sigma = GO._trilerp([GO._fetch(grid, k, density) for k in lk], wa[w_idx], wb[w_idx])[:, 0]
            hit = sigma > F(sigma_thresh)
            if hit.any():
                h_idx = w_idx[hit]
                rays = act[h_idx]
                lk_h = [k[hit] for k in lk]
                coef = GO._trilerp([GO._fetch(grid, k, sh) for k in lk_h], wa[h_idx], wb[h_idx]).reshape(-1, 3, B)
                raw = ((Y[rays][:, None, :] * coef).astype(F).sum(-1, dtype=F) + F(0.5)).astype(F)
                a = ((-step * sigma[hit]).astype(F) * delta_scale[rays]).astype(F)
                weight = (np.exp(log_t[rays]).astype(F) * (F(1.0) - np.exp(a).astype(F))).astype(F)
                rgb[rays] = (rgb[rays] + weight[:, None] * np.maximum(raw, F(0.0))).astype(F)
                tot[rays] += weight[:, None].astype(np.float64) * np.maximum(raw, F(0.0)).astype(np.float64)      # exact products
                log_t[rays] = (log_t[rays] + a).astype(F)
                if shade is not None:
                    shade(rays, lk_h, wa[h_idx], wb[h_idx], raw, weight, log_t[rays].copy())
                done = np.exp(log_t[rays]).astype(F) < F(stop_thresh)
                log_t[rays[done]] = F(-1e3)
                stopped[h_idx[done]] = True
        t0 = t[act].copy()
        t[act] = np.where(stopped, t[act], t_next)
        reach = (sv - 1).astype(F) - F(0.0625)
        going = ~work
        while going.any():
            cur = t[act]
            going &= (cur - t0).astype(F) <= reach
            nxt = (cur + step).astype(F)
            going &= nxt > cur
            t[act] = np.where(going, nxt, cur)
        keep = ~stopped
        keep &= t[act] <= tmax[act]
        act = act[keep]
    return rgb, log_t, (Y, delta_scale, marched, tot)


def fused(grid, origins, dirs, rgb_gt, step_size=0.5, sigma_thresh=1e-10, stop_thresh=1e-7, background_brightness=1.0,
          near_clip=0.0, skip=None, grad_density=None, grad_sh=None, mask=None, stats=None):
    """rgb_out [N, 3], grad_density [C, 1], grad_sh [C, 3 B], mask [C] uint8 of ``mean((rgb_out - rgb_gt) ** 2)``; the
    last three are added to when passed in. ``stats``: a dict that receives ``shaded`` (samples with sigma > sigma_thresh),
    ``clamped`` (those of them with a raw colour channel below 0) and ``marched`` (rays that were marched)."""
    cap, cols = grid["density_data"].shape[0], grid["sh_data"].shape[1]
    B = cols // 3
    gd = np.zeros((cap, 1), dtype=F) if grad_density is None else grad_density
    gs = np.zeros((cap, cols), dtype=F) if grad_sh is None else grad_sh
    mk = np.zeros(cap, dtype=np.uint8) if mask is None else mask
    args = (grid, origins, dirs, step_size, sigma_thresh, stop_thresh, near_clip, skip)
    rgb, log_t, (Y, delta_scale, marched, remaining) = _march(*args)
    rgb = (rgb + (np.exp(log_t).astype(F) * F(background_brightness))[:, None]).astype(F)
    # what the samples not yet passed and the background still add to each channel: fp64, reduced by the exact products below
    remaining += (np.exp(log_t).astype(F).astype(np.float64) * np.float64(F(background_brightness)))[:, None]
    n = rgb.shape[0]
    if n == 0:
        return rgb, gd, gs, mk
    scale = F(2.0) / (F(3.0) * F(n))
    gc = ((rgb - np.asarray(rgb_gt, F)).astype(F) * scale).astype(F)
    step_ds = (F(step_size) * delta_scale).astype(F)

    if stats is not None:
        stats.update(shaded=0, clamped=0, marched=int(marched.sum()))

    def shade(rays, lk, wa, wb, raw, weight, log_t_after):
        if stats is not None:
            stats["shaded"] += len(rays)
            stats["clamped"] += int((raw < 0).any(-1).sum())
        col = np.maximum(raw, F(0.0))
        g = gc[rays]
        dot = (((col[:, 0] * g[:, 0]).astype(F) + (col[:, 1] * g[:, 1]).astype(F)).astype(F) + (col[:, 2] * g[:, 2]).astype(F)).astype(F)
        remaining[rays] -= weight[:, None].astype(np.float64) * col.astype(np.float64)
        accum = (remaining[rays] * g.astype(np.float64)).sum(-1).astype(F)
        d_sigma = (step_ds[rays] * ((np.exp(log_t_after).astype(F) * dot).astype(F) - accum).astype(F)).astype(F)
        wy = (weight[:, None] * Y[rays]).astype(F)                                   # [n, B]
        d_coef = np.where(raw[:, :, None] >= 0, (wy[:, None, :] * g[:, :, None]).astype(F), F(0.0)).astype(F).reshape(-1, 3 * B)
        for c in range(8):
            wx = wb[:, 0] if c & 4 else wa[:, 0]
            wyy = wb[:, 1] if c & 2 else wa[:, 1]
            wz = wb[:, 2] if c & 1 else wa[:, 2]
            w8 = ((wx * wyy).astype(F) * wz).astype(F)
            kept = (lk[c] >= 0) & (lk[c] < cap)
            rows = lk[c][kept]
            np.add.at(gd[:, 0], rows, (w8 * d_sigma).astype(F)[kept])
            np.add.at(gs, rows, (w8[:, None] * d_coef).astype(F)[kept])
            mk[rows] = 1

    _march(*args, shade=shade)
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
