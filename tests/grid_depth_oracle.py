"""numpy restatement of the sparse voxel grid's depth and ray-length calls (include/nerf_mi355x.h, "Sparse voxel grid: depth
and ray lengths"), on the ray set-up and the sample lattice of tests/grid_oracle.py.

It states what csrc/grid_depth_kernels.hip computes with every operation a separate rounding in ``dtype``. fp32 mirrors the
kernels operation by operation. fp64 is the same statement on the same lattice: the set-up, the additions of ``t``, the
positions, cells and trilinear weights stay the fp32 ones of the header (as in tests/grid_resample_oracle.py); the density,
the exponentials, the weight, ``log_T`` and the depth are in fp64 - its distance from fp32 is what the roundings of the
accumulation are worth. A test oracle (not part of the package): slow and simple. Grids are the dicts of grid_oracle.
"""
import numpy as np

import grid_oracle as GO

F = np.float32


def ray_lengths(grid, origins, dirs, near_clip=0.0):
    """``tmax - tmin`` of the set-up in grid units (fp32): negative for a miss, NaN where the set-up is not finite."""
    _, _, _, _, tmin, tmax, ok = GO.ray_setup(grid, origins, dirs, near_clip)
    with np.errstate(invalid="ignore"):
        return np.where(ok, (tmax - tmin).astype(F), F(np.nan)).astype(F)


def depth(grid, origins, dirs, step_size=0.5, sigma_thresh=1e-10, stop_thresh=1e-7, near_clip=0.0, skip=None, threshold=None,
          dtype=F):
    """``(depth [N], log_transmit [N])`` in ``dtype``. ``threshold=None``: the expected termination under ``sigma_thresh`` /
    ``stop_thresh``. ``threshold=x``: the distance of the first sample whose density strictly exceeds ``x`` (``sigma_thresh`` and
    ``stop_thresh`` are not read, ``log_transmit`` stays 0). ``skip``: ``grid_oracle.skip_distances(links)`` or None."""
    if threshold is not None and not threshold >= 0:
        raise ValueError(f"threshold = {threshold!r} must be >= 0 and not NaN")
    links, density = grid["links"], grid["density_data"]
    step = F(step_size)
    o, g, _, delta_scale, tmin, tmax, ok = GO.ray_setup(grid, origins, dirs, near_clip)
    n = o.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        ds = delta_scale.astype(dtype)
        world_step = (dtype(step) * ds).astype(dtype)
    out = np.zeros(n, dtype=dtype)
    log_t = np.zeros(n, dtype=dtype)
    t = tmin.copy()
    with np.errstate(invalid="ignore"):
        skip_ok = (np.abs(o).max(-1) < GO.SKIP_MAX_T) & (np.abs(tmin) < GO.SKIP_MAX_T) & (np.abs(tmax) < GO.SKIP_MAX_T)
        act = np.nonzero(ok & (tmin <= tmax))[0]
    while act.size:
        # every pass advances t by at least one addition of step_size; a ray whose t no longer changes is left
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
            sigma = GO._trilerp([GO._fetch(grid, k, density).astype(dtype) for k in lk], wa[w_idx].astype(dtype),
                                wb[w_idx].astype(dtype))[:, 0]
            assert sigma.dtype == dtype
            hit = sigma > (dtype(F(sigma_thresh)) if threshold is None else dtype(F(threshold)))
            if hit.any():
                h_idx = w_idx[hit]
                rays = act[h_idx]
                steps = (t[rays].astype(dtype) / dtype(step)).astype(dtype)
                if threshold is not None:
                    out[rays] = (steps * world_step[rays]).astype(dtype)
                    stopped[h_idx] = True
                else:
                    a = ((-dtype(step) * sigma[hit]).astype(dtype) * ds[rays]).astype(dtype)
                    weight = (np.exp(log_t[rays]).astype(dtype) * (dtype(1.0) - np.exp(a).astype(dtype))).astype(dtype)
                    out[rays] = (out[rays] + ((weight * steps).astype(dtype) * world_step[rays]).astype(dtype)).astype(dtype)
                    log_t[rays] = (log_t[rays] + a).astype(dtype)
                    done = np.exp(log_t[rays]).astype(dtype) < dtype(F(stop_thresh))
                    log_t[rays[done]] = dtype(-1e3)
                    stopped[h_idx[done]] = True
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
    return out, log_t
