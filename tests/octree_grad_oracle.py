"""numpy oracle of the PlenOctree's backward (include/nerf_mi355x.h, "PlenOctree: backward"): a march that equals
``octree_oracle.march`` bit for bit and also records every pass's ``len = delta * delta_scale``, and the gradient of a ray's
colour with respect to the rows of ``data``, vectorised over rays, one pass per march step. The traversal is fp32 (the
definition); the radiometry and the gradient run in ``rad``: fp64 is the reference, fp32 - summed pass by pass, in ray order
within a pass - measures what fp32 arithmetic alone costs. A plain module."""
import numpy as np

import octree_oracle as O

# the stock cases with the sigma column multiplied by 8: on the stock cases almost no ray stops at stop_thresh = 1e-2
# (1 of 1024 on r8, none elsewhere); on these about two thirds do, with the same steps in fp32 and fp64 radiometry
DENSE = {"r8x8": ("r8", 8.0), "r16x8": ("r16", 8.0)}
_cache = {}


def case(name):
    """``O.case(name)``, or one of the dense cases; computed once and shared (do not write into them)."""
    if name not in DENSE:
        return O.case(name)
    if name not in _cache:
        base, mult = DENSE[name]
        grid, t, o, d = O.case(base)
        t = dict(t)
        data = t["data"].copy()
        data[..., -1] *= np.float32(mult)
        t["data"] = data
        _cache[name] = (grid, t, o, d)
    return _cache[name]


def march(tree, origins, dirs, step_size=1e-3, sigma_thresh=0.0, stop_thresh=0.0, background_brightness=1.0,
          rad=np.float32, max_iters=1 << 16):
    """``(rgb [n, 3] in rad, steps [n] int32, leaves [n, P] int64 padded with -1, lens [n, P] in rad, 0 where no leaf)``:
    ``octree_oracle.march`` with the fp32 traversal, operation for operation."""
    f, r = np.float32, np.dtype(rad).type
    child = tree["child"].reshape(-1).astype(np.int64)
    D = tree["data"].shape[-1]
    B = (D - 1) // 3
    data = tree["data"].reshape(-1, D)
    relu_half = tree["rgb_activation"] == "relu_half"
    ow = np.asarray(origins, np.float32)
    dw = np.asarray(dirs, np.float32)
    n = ow.shape[0]
    step = f(step_size)
    with np.errstate(all="ignore"):
        o = ow * tree["invradius"].astype(f) + tree["offset"].astype(f)
        d = dw * tree["invradius"].astype(f)
        ds = f(1) / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        d = d * ds[:, None]
        inv = f(1) / (d + f(1e-9))
        ok = np.isfinite(ow).all(1) & np.isfinite(dw).all(1) & np.isfinite(ds) & (ds > 0)
        tmin, tmax = O._unit(o, inv, f)
        basis = O.sh_basis(B, dw, rad)
        hi = f(np.float32(1.0) - np.float32(1e-6))
        active = ok & ~(tmax < 0) & ~(tmin > tmax)
        t = tmin.copy()
        T = np.ones(n, rad)
        rgb = np.zeros((n, 3), rad)
        steps = np.zeros(n, np.int32)
        done = np.zeros(n, bool)
        leaves, lens = [], []
        for it in range(max_iters):
            active = active & (t < tmax)
            idx = np.nonzero(active)[0]
            if idx.size == 0:
                break
            steps[idx] += 1
            p = np.fmin(np.fmax(o[idx] + t[idx, None] * d[idx], f(0)), hi)
            node = np.zeros(idx.size, np.int64)
            cell = np.zeros(idx.size, np.int64)
            inv_cube = np.ones(idx.size, f)
            live = np.ones(idx.size, bool)
            for _ in range(tree["max_depth"] + 1):
                p2 = p * f(2)
                u = (p2 >= f(1)).astype(np.int64)
                p = np.where(live[:, None], p2 - u.astype(f), p)
                inv_cube = np.where(live, inv_cube * f(0.5), inv_cube)
                cell = np.where(live, node * 8 + u[:, 0] * 4 + u[:, 1] * 2 + u[:, 2], cell)
                skip = child[cell]
                live = live & (skip != 0)
                node = np.where(live, node + skip, node)
                if not live.any():
                    break
            col = np.full(n, -1, np.int64)
            col[idx] = cell
            leaves.append(col)
            a, b = O._unit(p, inv[idx], f)
            delta = (b - a) * inv_cube + step
            ln = np.zeros(n, rad)
            ln[idx] = delta.astype(rad) * ds[idx].astype(rad)
            lens.append(ln)
            row = data[cell]
            sigma32 = row[:, D - 1]
            shade = sigma32 > np.float32(sigma_thresh)
            if shade.any():
                j = idx[shade]
                rw = row[shade].astype(rad)
                att = np.exp((-delta[shade].astype(rad) * ds[j].astype(rad)) * rw[:, D - 1])
                weight = T[j] * (r(1) - att)
                for c in range(3):
                    s = basis[j, 0] * rw[:, c * B]
                    for i in range(1, B):
                        s = s + basis[j, i] * rw[:, c * B + i]
                    colour = np.maximum(s + r(0.5), r(0)) if relu_half else r(1) / (r(1) + np.exp(-s))
                    rgb[j, c] = rgb[j, c] + weight * colour
                T[j] = T[j] * att
                stopped = j[T[j] <= r(np.float32(stop_thresh))]
                if stopped.size:
                    rgb[stopped] = rgb[stopped] * (r(1) / (r(1) - T[stopped]))[:, None]
                    done[stopped] = True
                    active[stopped] = False
            tn = t[idx] + delta
            adv = tn > t[idx]
            active[idx[~adv]] = False
            t[idx] = np.where(adv, tn, t[idx])
        else:
            raise AssertionError("a ray reached the cap of the march")
        add_bg = ok & ~done
        rgb[add_bg] = rgb[add_bg] + (T[add_bg] * r(np.float32(background_brightness)))[:, None]
        rgb[~ok] = np.nan
    lv = np.stack(leaves, 1) if leaves else np.zeros((n, 0), np.int64)
    ll = np.stack(lens, 1) if lens else np.zeros((n, 0), rad)
    return rgb, steps, lv, ll


def clamped_mse(rgb, gt):
    """``(loss, d loss / d rgb)`` of ``((clamp(rgb, 0, 1) - gt)**2).mean()`` over the rays that are not NaN (3 N counts every
    ray, as the package's fused form does); the derivative is 0 outside the closed interval [0, 1], torch.clamp's rule."""
    n = rgb.shape[0]
    ok = ~np.isnan(rgb).any(1)
    diff = np.where(ok[:, None], np.clip(rgb, 0.0, 1.0) - gt, 0.0)
    inside = (rgb >= 0.0) & (rgb <= 1.0)
    return (diff * diff).sum() / (3 * n), np.where(inside, diff * (2.0 / (3 * n)), 0.0)


def backward(tree, origins, dirs, g=None, rgb_gt=None, loss_scale=1.0, clamp_mask=True, rad=np.float64, data=None, **kw):
    """The header's block. ``g [n, 3]`` is the incoming gradient, or ``rgb_gt [n, 3]`` asks for the fused form
    (``g = loss_scale (clamp(rgb) - gt)`` where ``0 <= rgb <= 1``; ``clamp_mask=False`` drops that condition, to show what it
    does). ``data``: rows to use instead of the tree's (fp64 rows for the finite differences). Returns
    ``(rgb [n, 3], grad [cells, D] in rad, loss: the sum of squared clamped differences or None, stopped [n] bool)``."""
    r = np.dtype(rad).type
    if data is not None:
        tree = dict(tree)
        tree["data"] = data
    rgb, steps, lv, lens = march(tree, origins, dirs, rad=rad, **kw)
    D = tree["data"].shape[-1]
    B = (D - 1) // 3
    rows = tree["data"].reshape(-1, D)
    relu_half = tree["rgb_activation"] == "relu_half"
    n, P = lv.shape
    basis = O.sh_basis(B, np.asarray(dirs, np.float32), rad)
    sig_t, stop_t = np.float32(kw.get("sigma_thresh", 0.0)), r(np.float32(kw.get("stop_thresh", 0.0)))
    bg = r(np.float32(kw.get("background_brightness", 1.0)))
    valid = ~np.isnan(rgb).any(1)
    with np.errstate(all="ignore"):
        def shaded_rows(k):
            j = np.nonzero(lv[:, k] >= 0)[0]
            cell = lv[j, k]
            keep = rows[cell, D - 1] > sig_t
            j, cell = j[keep], cell[keep]
            return j, cell, rows[cell].astype(rad)

        def colours(j, rw):
            out = []
            for c in range(3):
                s = basis[j, 0] * rw[:, c * B]
                for i in range(1, B):
                    s = s + basis[j, i] * rw[:, c * B + i]
                if relu_half:
                    out.append((np.maximum(s + r(0.5), r(0)), ((s + r(0.5)) > 0).astype(rad)))
                else:
                    col = r(1) / (r(1) + np.exp(-s))
                    out.append((col, col * (r(1) - col)))
            return out

        # pass 1: the unscaled sums, the final transmittance, who stopped
        T = np.ones(n, rad)
        A = np.zeros((n, 3), rad)
        stopped = np.zeros(n, bool)
        for k in range(P):
            j, cell, rw = shaded_rows(k)
            if j.size == 0:
                continue
            att = np.exp(-lens[j, k] * rw[:, D - 1])
            w = T[j] * (r(1) - att)
            for c, (col, _) in enumerate(colours(j, rw)):
                A[j, c] = A[j, c] + w * col
            T[j] = T[j] * att
            stopped[j[T[j] <= stop_t]] = True
        scale = np.where(stopped, r(1) / (r(1) - T), r(1)).astype(rad)
        U = np.where(stopped[:, None], A, A + (T * bg)[:, None]).astype(rad)
        loss = None
        if rgb_gt is not None:
            gt = np.asarray(rgb_gt).astype(rad)
            diff = np.where(valid[:, None], np.clip(rgb, r(0), r(1)) - gt, r(0))
            loss = (diff * diff).sum()
            inside = (rgb >= 0) & (rgb <= 1) if clamp_mask else valid[:, None]
            g = np.where(inside, r(loss_scale) * diff, r(0))
        g = np.where(valid[:, None], np.asarray(g).astype(rad), r(0)).astype(rad)
        gs = g * scale[:, None]
        stop_term = np.where(stopped, -(g * A).sum(1) * scale * scale * T, r(0)).astype(rad)
        # pass 2: front to back with the running prefix
        grad = np.zeros(rows.shape, rad)
        Tk = np.ones(n, rad)
        pre = np.zeros((n, 3), rad)
        for k in range(P):
            j, cell, rw = shaded_rows(k)
            if j.size == 0:
                continue
            ln = lens[j, k]
            att = np.exp(-ln * rw[:, D - 1])
            w = Tk[j] * (r(1) - att)
            Ta = Tk[j] * att
            acc = stop_term[j].copy()
            contrib = np.empty((j.size, D), rad)
            for c, (col, dact) in enumerate(colours(j, rw)):
                wc = w * col
                acc = acc + gs[j, c] * (Ta * col - ((U[j, c] - pre[j, c]) - wc))
                kc = gs[j, c] * w * dact
                contrib[:, c * B:(c + 1) * B] = kc[:, None] * basis[j]
                pre[j, c] = pre[j, c] + wc
            contrib[:, D - 1] = ln * acc
            np.add.at(grad, cell, contrib)      # in ray order
            Tk[j] = Tk[j] * att
    return rgb, grad, loss, stopped


def shaded_cells(tree, origins, dirs, **kw):
    """bool ``[cells]``: the rows some ray shades (sigma above the threshold, at or before its stop)."""
    _, _, lv, _ = march(tree, origins, dirs, **kw)
    D = tree["data"].shape[-1]
    sigma = tree["data"].reshape(-1, D)[:, D - 1]
    cells = lv[lv >= 0]
    out = np.zeros(sigma.shape[0], bool)
    out[cells[sigma[cells] > np.float32(kw.get("sigma_thresh", 0.0))]] = True
    return out


def bar(got, g32, g64, B):
    """The GPU tests' bar, separately for the coefficient columns and the sigma column: ``max(3 d_ref, 1e-5 max|g64|)`` with
    ``d_ref`` the oracle's own fp32-to-fp64 distance (float atomics arrive in any order, hence the floor: the colour tests'
    1e-5 on values of order 1, scaled to the tensor). Returns ``[(largest difference, bar), (.., ..)]``."""
    out = []
    for sl in (slice(0, 3 * B), slice(3 * B, 3 * B + 1)):
        d_ref = np.abs(g32[:, sl].astype(np.float64) - g64[:, sl]).max()
        out.append((float(np.abs(got[:, sl].astype(np.float64) - g64[:, sl]).max()), float(max(3 * d_ref, 1e-5 * np.abs(g64[:, sl]).max()))))
    return out
