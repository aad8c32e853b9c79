"""numpy restatement of the background pass (include/nerf_mi355x.h, "Sparse voxel grid: background layers").

Stage by stage what csrc/grid_background_kernels.hip computes - the sphere set-up, the far hit of a radius, the texel
coordinates, the wrapped fetch with z, y, x interpolation, the compositing with its edge rules (``march``, the one
loop over the spheres, with a per-sphere ``shade`` hook: ``background_pass`` here, the taped pass and the backward of
grid_background_train_oracle.py) - in the dtype ``T``:
``np.float32`` with every operation a separate rounding (the kernel's arithmetic), or ``np.float64`` (the same formulas,
exact enough to measure the fp32 statement against). The radii and the inputs are the fp32 values in both. It starts where the
header starts: from the grid-coordinate origin ``o``, the unit grid direction ``d``, ``delta_scale`` and ``ok`` of the
foreground's set-up (``grid_oracle.ray_setup``). A test oracle (not part of the package): slow and simple.
A background is a dict: ``links`` int32 [2 R, R], ``data`` fp32 [capacity, L, 4].
"""
import numpy as np

F = np.float32
D = np.float64
SH_C0 = 0.28209479177387814
INV_PI = 0.318309886183790671538


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def setup(o, d, delta_scale, reso, T=F):
    """O, D (unit), world_step, q2a, qb, two_q2a, f, inner of every ray"""
    o, d, delta_scale = np.asarray(o, F).astype(T), np.asarray(d, F).astype(T), np.asarray(delta_scale, F).astype(T)
    s = T(2.0) / np.asarray(reso, F).astype(T)
    with np.errstate(all="ignore"):
        O = ((o + T(0.5)) * s) - T(1.0)
        Dv = d * s
        inorm = T(1.0) / np.sqrt(_dot(Dv, Dv))
        Dv = Dv * inorm[:, None]
        world_step = delta_scale * inorm
        q2a = T(2.0) * _dot(Dv, Dv)
        qb = T(2.0) * _dot(O, Dv)
        two_q2a = T(2.0) * q2a
        f = qb * qb - two_q2a * _dot(O, O)
        C = np.stack([O[:, 1] * Dv[:, 2] - O[:, 2] * Dv[:, 1], O[:, 2] * Dv[:, 0] - O[:, 0] * Dv[:, 2],
                      O[:, 0] * Dv[:, 1] - O[:, 1] * Dv[:, 0]], -1)
        inner = np.maximum(np.sqrt(_dot(C, C)) + T(1e-3), T(1.0))
    out = dict(O=O, D=Dv, world_step=world_step, q2a=q2a, qb=qb, two_q2a=two_q2a, f=f, inner=inner)
    assert all(v.dtype == T for v in out.values())
    return out


def radii(nlayers, step_size):
    """the n fp32 sphere radii of a render: n = int(float(L) / step_size) + 2, r_i = n / (n - i - 0.5) in fp64, rounded"""
    n = int(F(nlayers) / F(step_size)) + 2
    i = np.arange(n, dtype=D)
    return (D(n) / ((D(n) - i) - 0.5)).astype(F)


def hit(su, r, T=F):
    """the far hit of the sphere of radius ``r`` (one fp32 value): (taken [n] bool, t, invr, u [n, 3]); a ray is not taken
    where r < inner or det < 0"""
    r = T(F(r))
    with np.errstate(all="ignore"):
        det = su["f"] + (su["two_q2a"] * r) * r
        taken = ~(r < su["inner"]) & ~(det < 0)
        t = (-su["qb"] + np.sqrt(np.where(taken, det, T(0.0)))) / su["q2a"]
        P = su["O"] + t[:, None] * su["D"]
        invr = T(1.0) / np.sqrt(_dot(P, P))
        u = P * invr[:, None]
    return taken, t.astype(T), invr.astype(T), u.astype(T)


def texel_coords(u, invr, reso, nlayers, T=F):
    """x in [0, 2 R], y in [0, R], z in [0, L - 1]: x and y in fp64 from the angle in ``T``, rounded once to ``T``"""
    with np.errstate(all="ignore"):
        lat = np.arcsin(u[:, 1]).astype(T)
        lon = np.arctan2(u[:, 0], u[:, 2]).astype(T)
        x = (D(2 * reso) * (0.5 + (lon.astype(D) * 0.5) * INV_PI)).astype(T)
        y = (D(reso) * (0.5 - lat.astype(D) * INV_PI)).astype(T)
        z = np.fmin(np.fmax(((T(1.0) - invr) * T(nlayers)) - T(0.5), T(0.0)), T(nlayers - 1)).astype(T)
    return x, y, z


def cell(x, y, z, reso, nlayers, T=F):
    """l [n, 3] int (truncated, a NaN is 0, clamped to [0, (2 R - 1, R - 1, L - 2)]) and w = (x, y, z) - l"""
    hi = (2 * reso - 1, reso - 1, nlayers - 2)
    ls, ws = [], []
    for v, h in zip((x, y, z), hi):
        with np.errstate(all="ignore"):
            l = np.clip(np.where(np.isnan(v), 0.0, np.clip(v, -1.0, 1e6)).astype(np.int64), 0, h)
        ls.append(l)
        ws.append((v - l.astype(T)).astype(T))
    return np.stack(ls, -1), np.stack(ws, -1)


def _lerp(a, b, w):
    return a + w * (b - a)


def fetch(bg, l, w, T=F):
    """v [n, 4]: the four wrapped texels around l, each interpolated in z first, then y, then x; a texel without a row is 0"""
    links, data = bg["links"], np.asarray(bg["data"], F).astype(T)
    R2, R = links.shape
    L = data.shape[1]
    cap = data.shape[0]
    lx, ly, lz = l[:, 0], l[:, 1], l[:, 2]
    nx = np.where(lx < R2 - 1, lx + 1, 0)
    ny = np.where(ly < R - 1, ly + 1, 0)
    flat = links.reshape(-1)

    def texel(X, Y):
        lk = flat[X * R + Y].astype(np.int64)
        has = (lk >= 0) & (lk < cap)
        row = np.where(has, lk, 0)
        if cap == 0:
            return np.zeros((X.shape[0], 4), dtype=T)
        a, b = data[row, lz], data[row, np.minimum(lz + 1, L - 1)]
        return np.where(has[:, None], _lerp(a, b, w[:, 2:3]), T(0.0)).astype(T)

    v0 = _lerp(texel(lx, ly), texel(lx, ny), w[:, 1:2])
    v1 = _lerp(texel(nx, ly), texel(nx, ny), w[:, 1:2])
    return _lerp(v0, v1, w[:, 0:1]).astype(T)


def march(o, d, delta_scale, ok, reso, bg, log_in, step_size, stop_thresh, T, shade):
    """The one loop over the spheres, with its edge rules, for the rays with ``run`` = not left alone and a finite set-up, from
    ``log_in`` (in ``T``). ``shade(idx, l, w, v, dstep, weight, log_t_after)`` is called once per sphere with the rays shaded
    there. Returns (run, left_alone, final log_t, dict(stopped [n] bool, shaded [n] int))."""
    nl, R = bg["data"].shape[1], bg["links"].shape[1]
    ok = np.asarray(ok, bool)
    with np.errstate(invalid="ignore"):
        left_alone = log_in < T(-25.0)
    run = ~left_alone & ok
    su = setup(np.where(ok[:, None], o, 0.0), np.where(ok[:, None], d, 1.0), np.where(ok, delta_scale, 1.0), reso, T)
    log_t = log_in.copy()
    invr_last = (T(1.0) / su["inner"]).astype(T)
    live = run.copy()
    stats = dict(stopped=np.zeros(log_in.shape[0], bool), shaded=np.zeros(log_in.shape[0], np.int64))
    for r in radii(nl, step_size):
        taken, _, invr, u = hit(su, r, T)
        x, y, z = texel_coords(u, invr, R, nl, T)
        l, w = cell(x, y, z, R, nl, T)
        v = fetch(bg, l, w, T)
        cur = live & taken
        sh = cur & (v[:, 3] > 0)
        with np.errstate(all="ignore"):
            dstep = ((invr_last - invr) * su["world_step"]).astype(T)
            p = (dstep * v[:, 3]).astype(T)
            weight = (np.exp(log_t).astype(T) * (T(1.0) - np.exp(-p).astype(T))).astype(T)
            new_log = (log_t - p).astype(T)
            stop = sh & (np.exp(new_log).astype(T) < T(F(stop_thresh)))
        log_t = np.where(sh, new_log, log_t).astype(T)
        idx = np.nonzero(sh)[0]
        if idx.size:
            shade(idx, l[idx], w[idx], v[idx], dstep[idx], weight[idx], log_t[idx])
        stats["stopped"] |= stop
        stats["shaded"] += sh
        invr_last = np.where(cur & ~stop, invr, invr_last).astype(T)
        live = live & ~stop
    return run, left_alone, log_t, stats


def background_pass(o, d, delta_scale, ok, reso, bg, rgb, log_transmit, step_size=0.5, stop_thresh=1e-7,
                    background_brightness=1.0, T=F, return_stats=False):
    """(rgb [n, 3], log_transmit [n]) in ``T`` after the pass over a foreground's fp32 ``rgb`` / ``log_transmit``.
    ``return_stats``: also dict(left_alone, brightness_only, stopped [n] bool, shaded [n] int, seam [n] int)."""
    R = bg["links"].shape[1]
    rgb_in, log_in = np.asarray(rgb, F).astype(T), np.asarray(log_transmit, F).astype(T)
    n = rgb_in.shape[0]
    out = np.zeros((n, 3), T)
    seam = np.zeros(n, np.int64)

    def shade(idx, l, w, v, dstep, weight, log_t):
        col = np.maximum((v[:, :3] * T(SH_C0)) + T(0.5), T(0.0))
        out[idx] = (out[idx] + weight[:, None] * col).astype(T)
        seam[idx] += l[:, 0] == 2 * R - 1      # interpolated between the last and the first column

    run, left_alone, log_t, stats = march(o, d, delta_scale, ok, reso, bg, log_in, step_size, stop_thresh, T, shade)
    bright_only = ~left_alone & ~run
    with np.errstate(all="ignore"):
        full = rgb_in + (out + (np.exp(log_t).astype(T) * T(F(background_brightness)))[:, None])
        only = rgb_in + (np.exp(log_in).astype(T) * T(F(background_brightness)))[:, None]
    rgb_out = np.where(run[:, None], full, np.where(bright_only[:, None], only, rgb_in)).astype(T)
    log_out = np.where(run, log_t, log_in).astype(T)
    if return_stats:
        return rgb_out, log_out, dict(stats, left_alone=left_alone, brightness_only=bright_only, seam=seam)
    return rgb_out, log_out


def sparsify(bg, sigma_thresh=1.0, dilate=1):
    """(new links [2 R, R], new data): svox2's sparsify_background following each texel's own link"""
    links, data = bg["links"], bg["data"]
    cap, L = data.shape[0], data.shape[1]
    has = (links >= 0) & (links < cap)
    mask = np.zeros(links.shape + (L,), bool)
    with np.errstate(invalid="ignore"):
        mask[has] = data[links[has], :, 3] >= F(sigma_thresh)
    for _ in range(int(dilate)):
        p = np.pad(mask, 1, mode="edge")
        out = np.zeros_like(mask)
        X, Y, Z = mask.shape
        for a in range(3):
            for b in range(3):
                for c in range(3):
                    out |= p[a:a + X, b:b + Y, c:c + Z]
        mask = out
    keep = mask.any(-1) & has
    new_links = np.full(links.shape, -1, np.int32)
    new_links[keep] = np.arange(int(keep.sum()), dtype=np.int32)
    return new_links, data[links[keep]].astype(F).reshape(-1, L, 4)
