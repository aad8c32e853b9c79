"""numpy fp32 restatement of the sparse-voxel-grid renderer (include/nerf_mi355x.h, "Sparse voxel grid").

It states what csrc/grid_kernels.hip computes - ray set-up, the sample lattice, trilinear interpolation in the order z, y, x,
``sigma_thresh``, ``stop_thresh`` with ``log_T = -1e3``, the background term, non-finite rays, the stall rule, the skip distances and the jump - with every
operation a separate fp32 rounding, vectorised over rays. It is a test oracle (not part of the package): slow and simple.
Every foreground oracle walks its rays in ``march`` (csrc/grid_device.h's ``grid_march``: the lattice exists here only) and
interpolates with ``sigma_at`` and ``corner_weights``; ``march_colour`` is the colour accumulated along it, under ``render``
here and under the training and autograd oracles (grid_train_oracle.py, grid_autograd_oracle.py, grid_train_losses_oracle.py).
A grid is a dict: ``links`` int32 [X, Y, Z], ``density_data`` [C, 1], ``sh_data`` [C, 3 B], ``radius`` [3], ``center`` [3].
"""
import numpy as np

F = np.float32
SKIP_CAP = 32

SH_C0 = 0.28209479177387814
SH_C1 = 0.4886025119029199
SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)


def sh_bases(basis_dim, d):
    out = np.empty(d.shape[:-1] + (basis_dim,), dtype=d.dtype)
    c = d.dtype.type
    out[..., 0] = c(SH_C0)
    if basis_dim > 1:
        x, y, z = d[..., 0], d[..., 1], d[..., 2]
        out[..., 1] = c(-SH_C1) * y
        out[..., 2] = c(SH_C1) * z
        out[..., 3] = c(-SH_C1) * x
        if basis_dim > 4:
            xx, yy, zz = x * x, y * y, z * z
            out[..., 4] = c(SH_C2[0]) * (x * y)
            out[..., 5] = c(SH_C2[1]) * (y * z)
            out[..., 6] = c(SH_C2[2]) * (c(2.0) * zz - xx - yy)
            out[..., 7] = c(SH_C2[3]) * (x * z)
            out[..., 8] = c(SH_C2[4]) * (xx - yy)
    return out


def world2grid_consts(grid):
    gsz = np.array(grid["links"].shape, dtype=F)
    radius, center = np.asarray(grid["radius"], F), np.asarray(grid["center"], F)
    offset = (F(0.5) * (F(1.0) - center / radius)) * gsz - F(0.5)
    scaling = (F(0.5) / radius) * gsz
    return offset.astype(F), scaling.astype(F), gsz


def _fetch(table, links, dtype=F):
    """rows of ``table`` at ``links`` in ``dtype`` (any negative link or one >= capacity: zeros)"""
    ok = (links >= 0) & (links < table.shape[0])
    out = np.zeros((links.shape[0], table.shape[1]), dtype=dtype)
    out[ok] = table[links[ok]]
    return out


def _cell(pos, shape):
    """clamped position -> base cell l [n, 3] and weights wb [n, 3]"""
    hi = np.array(shape, dtype=F) - F(1.0)
    pos = np.minimum(np.maximum(pos, F(0.0)), hi).astype(F)
    l = np.minimum(pos.astype(np.int64), np.array(shape, dtype=np.int64) - 2)
    return l, (pos - l.astype(F)).astype(F)


def _corner_links(links, l):
    out = []
    for c in range(8):
        out.append(links[l[:, 0] + ((c >> 2) & 1), l[:, 1] + ((c >> 1) & 1), l[:, 2] + (c & 1)])
    return out


def _trilerp(v, wa, wb):
    """v: 8 arrays [n, C] in corner order 000, 001, ..., 111 (x, y, z bits); z, then y, then x"""
    z0, z1 = wa[:, 2:3], wb[:, 2:3]
    c00 = v[0] * z0 + v[1] * z1
    c01 = v[2] * z0 + v[3] * z1
    c10 = v[4] * z0 + v[5] * z1
    c11 = v[6] * z0 + v[7] * z1
    c0 = c00 * wa[:, 1:2] + c01 * wb[:, 1:2]
    c1 = c10 * wa[:, 1:2] + c11 * wb[:, 1:2]
    return c0 * wa[:, 0:1] + c1 * wb[:, 0:1]


def sigma_at(table, lk, wa, wb, dtype=F):
    """the density [n] in ``dtype`` interpolated from the density ``table`` [C, 1] (fp32, or fp64 for finite differences) at
    the corner links ``lk`` with the fp32 weights"""
    sigma = _trilerp([_fetch(table, k, dtype) for k in lk], wa.astype(dtype), wb.astype(dtype))[:, 0]
    assert sigma.dtype == dtype
    return sigma


def corner_weights(wa, wb, dtype=F):
    """(c, w8) with w8 the product (w_x * w_y) * w_z in ``dtype``, for the 8 corners in the order 000, 001, ..., 111 (x, y, z bits)"""
    wa, wb = wa.astype(dtype), wb.astype(dtype)
    for c in range(8):
        wx = wb[:, 0] if c & 4 else wa[:, 0]
        wy = wb[:, 1] if c & 2 else wa[:, 1]
        wz = wb[:, 2] if c & 1 else wa[:, 2]
        w8 = ((wx * wy).astype(dtype) * wz).astype(dtype)
        yield c, w8


def sample(grid, points, grid_coords=False, want_colors=True):
    links = grid["links"]
    p = np.asarray(points, dtype=F)
    if not grid_coords:
        offset, scaling, _ = world2grid_consts(grid)
        p = (offset + p * scaling).astype(F)
    l, wb = _cell(p, links.shape)
    wa = (F(1.0) - wb).astype(F)
    lk = _corner_links(links, l)
    dens = _trilerp([_fetch(grid["density_data"], k) for k in lk], wa, wb)
    if not want_colors:
        return dens, np.zeros((0, grid["sh_data"].shape[1]), dtype=F)
    return dens, _trilerp([_fetch(grid["sh_data"], k) for k in lk], wa, wb)


def skip_distances(links):
    """uint8 [X, Y, Z] indexed by a cell's lowest node: 0 = a corner of the cell is kept; v >= 1 = every node within v - 1
    cells (Chebyshev, clipped to the grid) of the cell's corners is empty; capped at SKIP_CAP."""
    X, Y, Z = links.shape
    empty = links < 0
    cell = np.ones((X - 1, Y - 1, Z - 1), dtype=bool)
    for c in range(8):
        a, b, d = (c >> 2) & 1, (c >> 1) & 1, c & 1
        cell &= empty[a:a + X - 1, b:b + Y - 1, d:d + Z - 1]
    dist = cell.astype(np.uint8)
    for r in range(1, SKIP_CAP):
        ge = np.pad(dist >= r, 1, constant_values=True)      # outside the grid does not constrain
        ok = np.ones_like(cell)
        for a in range(3):
            for b in range(3):
                for d in range(3):
                    ok &= ge[a:a + X - 1, b:b + Y - 1, d:d + Z - 1]
        dist[(dist == r) & ok] = r + 1
    out = np.zeros((X, Y, Z), dtype=np.uint8)
    out[:X - 1, :Y - 1, :Z - 1] = dist
    return out


SKIP_MAX_T = F(131072.0)      # 2^17: skip data is used only while |origin| and |t| (grid units) stay below it


def ray_setup(grid, origins, dirs, near_clip=0.0):
    """o, d (grid units, unit), view direction, delta_scale, tmin, tmax, and ok: the set-up is finite (a zero, NaN or
    infinite direction or origin is a miss)"""
    offset, scaling, gsz = world2grid_consts(grid)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        o = (offset + np.asarray(origins, F) * scaling).astype(F)
        d = np.asarray(dirs, F)
        dn = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F)
        view = (d / dn[:, None]).astype(F)
        g = (view * scaling).astype(F)
        delta_scale = (F(1.0) / np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]).astype(F)).astype(F)
        g = (g * delta_scale[:, None]).astype(F)
        inv = (F(1.0) / g).astype(F)
        t1 = ((F(-0.5) - o) * inv).astype(F)
        t2 = ((gsz - F(0.5) - o) * inv).astype(F)
        lo, hi = np.fmin(t1, t2), np.fmax(t1, t2)      # (fminf / fmaxf: a NaN operand is dropped)
        lo[g == 0] = F(-1e9)
        hi[g == 0] = F(1e9)
        tmin = np.fmax(np.fmax(np.fmax(np.fmax(F(-1e9), lo[:, 0]), lo[:, 1]), lo[:, 2]), F(near_clip)).astype(F)
        tmax = np.fmin(np.fmin(np.fmin(F(1e9), hi[:, 0]), hi[:, 1]), hi[:, 2]).astype(F)
        ok = (dn > 0) & np.isfinite(dn) & np.isfinite(delta_scale) & np.isfinite(tmin) & np.isfinite(tmax) \
            & np.isfinite(o).all(-1) & np.isfinite(g).all(-1)
    return o, g, view, delta_scale, tmin, tmax, ok


def march(grid, origins, dirs, at, step_size=0.5, near_clip=0.0, skip=None):
    """grid_march of csrc/grid_device.h, the one sample lattice of the foreground oracles. ``at(rays, t, lk, wa, wb)`` is called
    once per pass with the samples whose links are loaded - every sample the skip rule does not pass over; a ray at most once per
    pass, passes in march order - ``lk`` the 8 corner-link arrays, ``wa`` / ``wb`` the fp32 weights. It applies its own density
    threshold and returns the mask of the rays that end. Returns the rays that were marched [N] bool."""
    links = grid["links"]
    step = F(step_size)
    o, g, _, _, tmin, tmax, ok = ray_setup(grid, origins, dirs, near_clip)
    t = tmin.copy()
    with np.errstate(invalid="ignore"):
        skip_ok = (np.abs(o).max(-1) < SKIP_MAX_T) & (np.abs(tmin) < SKIP_MAX_T) & (np.abs(tmax) < SKIP_MAX_T)
        marched = ok & (tmin <= tmax)
    act = np.nonzero(marched)[0]
    while act.size:
        # every pass advances t by at least one addition of step_size; a ray whose t no longer changes is left
        t_next = (t[act] + step).astype(F)
        act, t_next = act[t_next > t[act]], t_next[t_next > t[act]]
        if not act.size:
            break
        pos = (o[act] + t[act, None] * g[act]).astype(F)
        l, wb = _cell(pos, links.shape)
        wa = (F(1.0) - wb).astype(F)
        sv = np.zeros(act.size, dtype=np.int64)
        if skip is not None:
            sv = np.where(skip_ok[act], skip[l[:, 0], l[:, 1], l[:, 2]].astype(np.int64), 0)
        work = sv == 0
        stopped = np.zeros(act.size, dtype=bool)
        if work.any():
            w_idx = np.nonzero(work)[0]
            lk = [k[w_idx] for k in _corner_links(links, l)]
            stopped[w_idx] = at(act[w_idx], t[act[w_idx]], lk, wa[w_idx], wb[w_idx])
        t0 = t[act].copy()
        t[act] = np.where(stopped, t[act], t_next)
        # a skipping ray also passes every later sample whose accumulated t is within sv - 1 - 1/16 of this one's
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
    return marched


def view_bases(grid, origins, dirs, near_clip=0.0):
    """what a colour march needs of the rays alone: the SH bases Y [N, B] of the view direction (of the zero direction where
    the set-up is not finite) and delta_scale [N]"""
    _, _, view, delta_scale, _, _, ok = ray_setup(grid, origins, dirs, near_clip)
    return sh_bases(grid["sh_data"].shape[1] // 3, np.where(ok[:, None], view, F(0.0)).astype(F)), delta_scale


def march_colour(grid, origins, dirs, step_size=0.5, sigma_thresh=1e-10, stop_thresh=1e-7, near_clip=0.0, skip=None, shade=None):
    """march_colour of csrc/grid_device.h on :func:`march`. Returns (rgb without the background term, log_transmit, (Y,
    delta_scale, marched, the same colour summed in fp64), (samples whose links were loaded, samples shaded)).
    ``shade(rays, lk, wa, wb, sigma, raw, weight, log_t_after)`` is called once per pass with the shaded samples of that pass."""
    density, sh = grid["density_data"], grid["sh_data"]
    B = sh.shape[1] // 3
    step = F(step_size)
    Y, delta_scale = view_bases(grid, origins, dirs, near_clip)
    n = Y.shape[0]
    rgb = np.zeros((n, 3), dtype=F)
    tot = np.zeros((n, 3), dtype=np.float64)      # the colour once more, as the fp64 sum of its exact terms
    log_t = np.zeros(n, dtype=F)
    count = [0, 0]

    def at(rays, t, lk, wa, wb):
        count[0] += rays.size
        sigma = sigma_at(density, lk, wa, wb)
        hit = sigma > F(sigma_thresh)
        done = np.zeros(rays.size, dtype=bool)
        if hit.any():
            rays, lk, wa, wb, sigma = rays[hit], [k[hit] for k in lk], wa[hit], wb[hit], sigma[hit]
            count[1] += rays.size
            coef = _trilerp([_fetch(sh, k) for k in lk], wa, wb).reshape(-1, 3, B)
            raw = ((Y[rays][:, None, :] * coef).astype(F).sum(-1, dtype=F) + F(0.5)).astype(F)
            col = np.maximum(raw, F(0.0))
            a = ((-step * sigma).astype(F) * delta_scale[rays]).astype(F)
            weight = (np.exp(log_t[rays]).astype(F) * (F(1.0) - np.exp(a).astype(F))).astype(F)
            rgb[rays] = (rgb[rays] + weight[:, None] * col).astype(F)
            tot[rays] += weight[:, None].astype(np.float64) * col.astype(np.float64)      # exact products
            log_t[rays] = (log_t[rays] + a).astype(F)
            if shade is not None:
                shade(rays, lk, wa, wb, sigma, raw, weight, log_t[rays].copy())
            end = np.exp(log_t[rays]).astype(F) < F(stop_thresh)
            log_t[rays[end]] = F(-1e3)
            done[hit] = end
        return done

    marched = march(grid, origins, dirs, at, step_size, near_clip, skip)
    return rgb, log_t, (Y, delta_scale, marched, tot), tuple(count)


def render(grid, origins, dirs, step_size=0.5, sigma_thresh=1e-10, stop_thresh=1e-7, background_brightness=1.0,
           near_clip=0.0, skip=None, return_counts=False):
    """rgb [N, 3], log_transmit [N] (and (samples whose links were loaded, samples shaded))."""
    rgb, log_t, _, counts = march_colour(grid, origins, dirs, step_size, sigma_thresh, stop_thresh, near_clip, skip)
    rgb = (rgb + (np.exp(log_t).astype(F) * F(background_brightness))[:, None]).astype(F)
    return (rgb, log_t, counts) if return_counts else (rgb, log_t)


def gen_rays(c2w, fx, fy, cx, cy, width, height):
    """svox2 Camera.gen_rays without NDC: fp64, rounded to fp32. c2w [3, 4] OpenCV."""
    c2w = np.asarray(c2w, dtype=np.float32)[:3, :4]
    yy, xx = np.meshgrid(np.arange(height, dtype=np.float64) + 0.5, np.arange(width, dtype=np.float64) + 0.5, indexing="ij")
    d = np.stack([(xx - cx) / fx, (yy - cy) / fy, np.ones_like(xx)], -1).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    dirs = (d @ c2w[:, :3].astype(np.float64).T).astype(np.float32)
    origins = np.broadcast_to(c2w[None, :, 3], dirs.shape).copy()
    return origins, dirs
