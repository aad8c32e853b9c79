"""numpy restatement of the sparse voxel grid's depth and ray-length calls (include/nerf_mi355x.h, "Sparse voxel grid: depth
and ray lengths"), on the ray set-up and the sample lattice of tests/grid_oracle.py: ``depth`` is a callback of its ``march``.

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
    step = dtype(F(step_size))
    _, _, _, delta_scale, _, _, _ = GO.ray_setup(grid, origins, dirs, near_clip)
    with np.errstate(invalid="ignore", over="ignore"):
        ds = delta_scale.astype(dtype)
        world_step = (step * ds).astype(dtype)
    out = np.zeros(ds.shape[0], dtype=dtype)
    log_t = np.zeros(ds.shape[0], dtype=dtype)

    def at(rays, t, lk, wa, wb):
        sigma = GO.sigma_at(grid["density_data"], lk, wa, wb, dtype)
        hit = sigma > (dtype(F(sigma_thresh)) if threshold is None else dtype(F(threshold)))
        rays, sigma, done = rays[hit], sigma[hit], hit.copy()      # (threshold mode: the first hit ends the ray)
        steps = (t[hit].astype(dtype) / step).astype(dtype)
        if threshold is not None:
            out[rays] = (steps * world_step[rays]).astype(dtype)
        else:
            a = ((-step * sigma).astype(dtype) * ds[rays]).astype(dtype)
            weight = (np.exp(log_t[rays]).astype(dtype) * (dtype(1.0) - np.exp(a).astype(dtype))).astype(dtype)
            out[rays] = (out[rays] + ((weight * steps).astype(dtype) * world_step[rays]).astype(dtype)).astype(dtype)
            log_t[rays] = (log_t[rays] + a).astype(dtype)
            end = np.exp(log_t[rays]).astype(dtype) < dtype(F(stop_thresh))
            log_t[rays[end]] = dtype(-1e3)
            done[hit] = end
        return done

    GO.march(grid, origins, dirs, at, step_size, near_clip, skip)
    return out, log_t
