"""numpy restatement of the gradients of the sparse voxel grid's expected depth and log_transmit (include/nerf_mi355x.h,
"Sparse voxel grid: gradients of depth and log_transmit for autograd"): the taped forward and the backward with a cotangent
for each result, both callbacks of ``march`` of tests/grid_oracle.py (its ray set-up, its sample lattice, its ``sigma_at`` and
``corner_weights``). The taped forward must reproduce the expected depth of tests/grid_depth_oracle.py bit for bit
(tests/test_grid_depth_autograd_cpu.py).

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


def _shaded(at, density, sigma_thresh, dtype):
    """the callback of grid_oracle.march that calls ``at(rays, t, lk, wa, wb, sigma)`` with the samples of a pass whose sigma (in
    ``dtype``, of the table ``density``) exceeds ``sigma_thresh``; ``at`` returns the mask of the rays that stop"""
    def of_pass(rays, t, lk, wa, wb):
        sigma = GO.sigma_at(density, lk, wa, wb, dtype)
        hit = sigma > dtype(F(sigma_thresh))
        done = np.zeros(rays.size, dtype=bool)
        if hit.any():
            done[hit] = at(rays[hit], t[hit], [k[hit] for k in lk], wa[hit], wb[hit], sigma[hit])
        return done
    return of_pass


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
        GO.march(grid, origins, dirs, _shaded(at, density, sigma_thresh, dtype), step_size, near_clip, skip)
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
        for c, w8 in GO.corner_weights(wa, wb, dtype):
            kept = (lk[c] >= 0) & (lk[c] < gd.shape[0])
            np.add.at(gd[:, 0], lk[c][kept], (w8 * d_sigma).astype(dtype)[kept])
        return np.exp(log_t[rays]).astype(dtype) < dtype(F(stop_thresh))

    with np.errstate(over="ignore", invalid="ignore"):
        GO.march(grid, origins, dirs, _shaded(at, density, sigma_thresh, dtype), step_size, near_clip, skip)
    return gd


def depth_vjp(grid, origins, dirs, grad_depth=None, grad_log_transmit=None, **kw):
    """taped forward, then the backward: ``(depth, log_transmit, grad_density)``. A cotangent is an array, None, or a callable
    of ``(depth, log_transmit)``."""
    fwd = {k: v for k, v in kw.items() if k != "grad_density"}
    depth, log_t, tape = depth_taped(grid, origins, dirs, **fwd)
    g_d = grad_depth(depth, log_t) if callable(grad_depth) else grad_depth
    g_t = grad_log_transmit(depth, log_t) if callable(grad_log_transmit) else grad_log_transmit
    return depth, log_t, depth_backward(grid, origins, dirs, g_d, g_t, None if g_d is None else tape, **kw)
