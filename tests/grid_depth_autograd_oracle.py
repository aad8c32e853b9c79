"""numpy restatement of the gradients of the sparse voxel grid's expected depth and log_transmit (include/nerf_mi355x.h,
"Sparse voxel grid: gradients of depth and log_transmit for autograd"): the taped forward and the backward with a cotangent
for each result, on the ray set-up of tests/grid_oracle.py and the sample lattice of tests/grid_depth_oracle.py (whose
expected depth the taped forward here must reproduce bit for bit: tests/test_grid_depth_autograd_cpu.py).

``dtype=np.float32`` mirrors csrc/grid_depth_autograd_kernels.hip: every operation a separate fp32 rounding in the header's
order, ``remaining`` in fp64. ``dtype=np.float64`` is the same statement on the same lattice - set-up, additions of ``t``,
positions, cells and trilinear weights stay the fp32 ones - with the density, the exponentials, the weights and the sums in
fp64, and may be given a ``density`` table in fp64 (finite differences). Sums into a gradient row are taken in sample order
(the kernel's atomics take them in any order), so gradients agree with the kernel to rounding of those sums. A test oracle
(not part of the package): slow and simple. Grids are the dicts of grid_oracle.
"""
import numpy as np

import grid_oracle as GO

F = np.float32


def _rows(table, links, dtype):
    """``table[links]`` in ``dtype``, zeros where a link is negative or >= capacity"""
    ok = (links >= 0) & (links < table.shape[0])
    out = np.zeros(links.shape[0], dtype=dtype)
    out[ok] = table[links[ok], 0]
    return out


def _march(grid, origins, dirs, step_size, sigma_thresh, near_clip, skip, dtype, density, at):
    """The lattice of grid_depth_oracle.depth: ``at(rays, t, lk, wa, wb, sigma)`` at the samples with sigma > sigma_thresh of
    one pass (every ray at most once per pass, passes in march order); it returns the mask of the rays that stop."""
    links = grid["links"]
    step = F(step_size)
    o, g, _, _, tmin, tmax, ok = GO.ray_setup(grid, origins, dirs, near_clip)
    t = tmin.copy()
    with np.errstate(invalid="ignore"):
        skip_ok = (np.abs(o).max(-1) < GO.SKIP_MAX_T) & (np.abs(tmin) < GO.SKIP_MAX_T) & (np.abs(tmax) < GO.SKIP_MAX_T)
        act = np.nonzero(ok & (tmin <= tmax))[0]
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
            sigma = GO._trilerp([_rows(density, k, dtype)[:, None] for k in lk], wa[w_idx].astype(dtype), wb[w_idx].astype(dtype))[:, 0]
            assert sigma.dtype == dtype
            hit = sigma > dtype(F(sigma_thresh))
            if hit.any():
                h_idx = w_idx[hit]
                done = at(act[h_idx], t[act[h_idx]], [k[hit] for k in lk], wa[h_idx], wb[h_idx], sigma[hit])
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


class _Ray:
    """what the forward and the backward share per ray: delta_scale and world_step in ``dtype``, and the sample's terms"""

    def __init__(self, grid, origins, dirs, step_size, near_clip, dtype):
        _, _, _, delta_scale, _, _, _ = GO.ray_setup(grid, origins, dirs, near_clip)
        self.dtype, self.step = dtype, dtype(F(step_size))
        with np.errstate(invalid="ignore", over="ignore"):
            self.ds = delta_scale.astype(dtype)
            self.world_step = (self.step * self.ds).astype(dtype)

    def terms(self, rays, t, sigma, log_t):
        """a, tau, term = (weight * tau) * world_step of a pass"""
        dt = self.dtype
        a = ((-self.step * sigma).astype(dt) * self.ds[rays]).astype(dt)
        weight = (np.exp(log_t[rays]).astype(dt) * (dt(1.0) - np.exp(a).astype(dt)).astype(dt)).astype(dt)
        tau = (t.astype(dt) / self.step).astype(dt)
        return a, tau, ((weight * tau).astype(dt) * self.world_step[rays]).astype(dt)


def _forward(grid, origins, dirs, step_size, sigma_thresh, stop_thresh, near_clip, skip, dtype, density):
    density = grid["density_data"] if density is None else density
    n = np.asarray(origins).shape[0]
    depth, log_t = np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype)
    tape, stopped = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=bool)
    if n == 0:
        return depth, log_t, tape, stopped
    ray = _Ray(grid, origins, dirs, step_size, near_clip, dtype)

    def at(rays, t, lk, wa, wb, sigma):
        a, _, term = ray.terms(rays, t, sigma, log_t)
        depth[rays] = (depth[rays] + term).astype(dtype)
        tape[rays] += term.astype(np.float64)
        log_t[rays] = (log_t[rays] + a).astype(dtype)
        done = np.exp(log_t[rays]).astype(dtype) < dtype(F(stop_thresh))
        log_t[rays[done]] = dtype(-1e3)
        stopped[rays[done]] = True
        return done

    with np.errstate(over="ignore", invalid="ignore"):
        _march(grid, origins, dirs, step_size, sigma_thresh, near_clip, skip, dtype, density, at)
    return depth, log_t, tape, stopped


def depth_taped(grid, origins, dirs, step_size=0.5, sigma_thresh=1e-10, stop_thresh=1e-7, near_clip=0.0, skip=None, dtype=F,
                density=None):
    """``(depth [N], log_transmit [N])`` in ``dtype`` and ``tape [N]`` in fp64"""
    return _forward(grid, origins, dirs, step_size, sigma_thresh, stop_thresh, near_clip, skip, dtype, density)[:3]


def depth_backward(grid, origins, dirs, grad_depth, grad_log_transmit, tape, step_size=0.5, sigma_thresh=1e-10,
                   stop_thresh=1e-7, near_clip=0.0, skip=None, dtype=F, density=None, grad_density=None):
    """``grad_density [C, 1]`` of ``sum(grad_depth * depth) + sum(grad_log_transmit * log_transmit)``, added to when passed
    in; either cotangent may be None, ``tape`` is None with ``grad_depth``"""
    if grad_depth is None and grad_log_transmit is None:
        raise ValueError("grad_depth and grad_log_transmit are both None")
    if (grad_depth is None) != (tape is None):
        raise ValueError("tape must be None if and only if grad_depth is None")
    density = grid["density_data"] if density is None else density
    gd = np.zeros((density.shape[0], 1), dtype=dtype) if grad_density is None else grad_density
    n = np.asarray(origins).shape[0]
    if n == 0:
        return gd
    g_d = np.zeros(n, dtype=dtype) if grad_depth is None else np.asarray(grad_depth, dtype).reshape(n)
    g_t = np.zeros(n, dtype=dtype) if grad_log_transmit is None else np.asarray(grad_log_transmit, dtype).reshape(n).copy()
    # a ray that stops returned the constant -1e3: its log_transmit has no gradient
    g_t[_forward(grid, origins, dirs, step_size, sigma_thresh, stop_thresh, near_clip, skip, dtype, density)[3]] = 0
    remaining = np.zeros(n, dtype=np.float64) if tape is None else np.array(tape, dtype=np.float64).reshape(n)
    log_t = np.zeros(n, dtype=dtype)
    ray = _Ray(grid, origins, dirs, step_size, near_clip, dtype)
    step_ds = ray.world_step

    def at(rays, t, lk, wa, wb, sigma):
        a, tau, term = ray.terms(rays, t, sigma, log_t)
        remaining[rays] -= term.astype(np.float64)
        log_t[rays] = (log_t[rays] + a).astype(dtype)
        lead = ((np.exp(log_t[rays]).astype(dtype) * tau).astype(dtype) * ray.world_step[rays]).astype(dtype)
        inner = (g_d[rays] * (lead - remaining[rays].astype(dtype)).astype(dtype)).astype(dtype)
        d_sigma = ((step_ds[rays] * inner).astype(dtype) - (g_t[rays] * step_ds[rays]).astype(dtype)).astype(dtype)
        wa, wb = wa.astype(dtype), wb.astype(dtype)
        for c in range(8):
            wx = wb[:, 0] if c & 4 else wa[:, 0]
            wy = wb[:, 1] if c & 2 else wa[:, 1]
            wz = wb[:, 2] if c & 1 else wa[:, 2]
            w8 = ((wx * wy).astype(dtype) * wz).astype(dtype)
            kept = (lk[c] >= 0) & (lk[c] < gd.shape[0])
            np.add.at(gd[:, 0], lk[c][kept], (w8 * d_sigma).astype(dtype)[kept])
        return np.exp(log_t[rays]).astype(dtype) < dtype(F(stop_thresh))

    with np.errstate(over="ignore", invalid="ignore"):
        _march(grid, origins, dirs, step_size, sigma_thresh, near_clip, skip, dtype, density, at)
    return gd


def depth_vjp(grid, origins, dirs, grad_depth=None, grad_log_transmit=None, **kw):
    """taped forward, then the backward: ``(depth, log_transmit, grad_density)``. A cotangent is an array, None, or a callable
    of ``(depth, log_transmit)``."""
    fwd = {k: v for k, v in kw.items() if k != "grad_density"}
    depth, log_t, tape = depth_taped(grid, origins, dirs, **fwd)
    g_d = grad_depth(depth, log_t) if callable(grad_depth) else grad_depth
    g_t = grad_log_transmit(depth, log_t) if callable(grad_log_transmit) else grad_log_transmit
    return depth, log_t, depth_backward(grid, origins, dirs, g_d, g_t, None if g_d is None else tape, **kw)
