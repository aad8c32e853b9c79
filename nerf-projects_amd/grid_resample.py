"""Resampling a sparse voxel grid (Plenoxels): change the resolution and the set of kept nodes, for coarse-to-fine training.

``resample_grid(grid, reso, ...)`` is svox2's ``SparseGrid.resample`` with its arguments and defaults, through the HIP
kernels of csrc/grid_resample_kernels.hip; the semantics of every stage are stated in include/nerf_mi355x.h, "Sparse voxel
grid: resampling". It returns a new grid; ``GridTrainer.resample`` does the same in place inside a training loop. The
mapping::

    svox2                                              here
    grid.resample(reso, sigma_thresh, ...)             new = resample_grid(grid, reso, sigma_thresh, ...)
                                                       trainer.resample(reso, sigma_thresh, ...)      (in place)
    _C.grid_weight_render(volume, cam, 0.5, ...)       weight_render(volume, camera, radius, center, ...)
    _C.dilate(mask)                                    dilate_mask(mask)
    torch.linspace lattice + grid.sample(points)       lattice_axes(...) + lattice_density(grid, axes)

``SparseGrid.resample`` itself still raises ``NotImplementedError``, like the other svox2-named training methods.
``use_z_order`` is not offered (rows come out in C order), background layers and ``last_sample_opaque`` are not built.
There is no CPU or PyTorch fallback. The kept-node count is read from the device once, to allocate the new tables: that is
the only wait of a resample (``max_elements > 0``, a cold path in torch as in svox2, adds two: the count of nodes that pass
the threshold and, when that exceeds ``max_elements``, the top-k threshold).
"""
import ctypes as C

import numpy as np
import torch

from ._lib import GridCompactArgs, GridGatherArgs, GridLatticeArgs, GridWeightArgs, check
from .grid import Camera, SparseGrid, _as_u8, _refuse_half, _reso3, _three, _volume_arg
from .host import get_context

__all__ = ["resample_grid", "lattice_axes", "lattice_density", "weight_render", "threshold_mask", "dilate_mask", "compact_mask"]

def lattice_axes(old_reso, reso):
    """The node coordinates of a lattice of ``reso`` in the coordinates of a grid of ``old_reso``, per axis, as svox2 makes
    them: ``torch.linspace(f - 0.5, R - f - 0.5, R')`` with ``f = 0.5 R / R'``, fp32, on the CPU."""
    out = []
    for r_old, r_new in zip(old_reso, reso):
        f = 0.5 * r_old / r_new
        out.append(torch.linspace(f - 0.5, r_old - f - 0.5, r_new, dtype=torch.float32))
    return out


def _axes_arg(axes, reso, ctx):
    out = []
    for a, r in zip(axes, reso):
        a = torch.as_tensor(a)
        if a.dim() != 1 or a.shape[0] != r:
            raise ValueError(f"a lattice axis must be [{r}], got {tuple(a.shape)}")
        out.append(a.detach().to(device=ctx.device, dtype=torch.float32).contiguous())
    return out


def lattice_density(grid, axes):
    """``[X', Y', Z']``: the density of ``grid`` at the lattice whose per-axis coordinates (in ``grid``'s own coordinates)
    are the three 1-D tensors ``axes``; bit for bit ``grid.sample(points, grid_coords=True)`` at the same points."""
    if not isinstance(grid, SparseGrid):
        raise TypeError("lattice_density needs a SparseGrid")
    if len(axes) != 3:
        raise ValueError("axes: three 1-D tensors")
    reso = _reso3([int(torch.as_tensor(a).numel()) for a in axes], "the lattice")
    ctx = grid.ctx
    ax = _axes_arg(axes, reso, ctx)
    h = grid._handle()
    vol = torch.empty(reso, dtype=torch.float32, device=ctx.device)
    a = GridLatticeArgs()
    a.reso[:] = reso
    a.xs, a.ys, a.zs, a.density = ax[0].data_ptr(), ax[1].data_ptr(), ax[2].data_ptr(), vol.data_ptr()
    a.stream = ctx.stream().value
    check(ctx.lib.nerf_grid_lattice_density(h, C.byref(a)))
    return vol


def weight_render(density_volume, camera, radius, center, step_size=0.5, stop_thresh=0.2, last_sample_opaque=False, out=None):
    """svox2's ``grid_weight_render``: march the rays of ``camera`` through the dense ``density_volume`` ``[X, Y, Z]`` of a
    grid with ``radius`` / ``center`` and raise ``out`` (a new zero volume when ``None``) at the 8 corners of every sample to
    the sample's rendering weight. Returns ``out``. Deterministic: the maximum is an integer atomic on the weight's bits,
    which orders floats correctly only when they are non-negative: a caller's ``out`` must hold no negative value and no
    NaN (a volume of zeros, or the result of earlier calls; it is not checked, that would wait for the device)."""
    if last_sample_opaque:
        raise NotImplementedError("last_sample_opaque is not built")
    if not isinstance(camera, Camera):
        raise TypeError("weight_render needs a grid Camera")
    vol = _volume_arg(density_volume, "density_volume", torch.float32)
    ctx = get_context(vol.device)
    reso = list(vol.shape)
    if out is None:
        out = torch.zeros(reso, dtype=torch.float32, device=ctx.device)
    else:
        _volume_arg(out, "out", torch.float32, ctx)
        if not out.is_contiguous() or list(out.shape) != reso:
            raise ValueError(f"out must be a contiguous float32 {reso} volume")
    cam = camera._to_c()
    a = GridWeightArgs()
    a.reso[:] = reso
    a.radius[:] = _three(radius, "radius").tolist()
    a.center[:] = _three(center, "center").tolist()
    a.density, a.max_weight = vol.data_ptr(), out.data_ptr()
    a.step_size, a.stop_thresh, a.last_sample_opaque = float(step_size), float(stop_thresh), 0
    a.stream = ctx.stream().value
    check(ctx.lib.nerf_grid_weight_render(ctx.handle, C.byref(cam), C.byref(a)))
    return out


def threshold_mask(volume, threshold):
    """``volume >= threshold`` as a uint8 ``[X, Y, Z]`` mask."""
    vol = _volume_arg(volume, "volume", torch.float32)
    ctx = get_context(vol.device)
    mask = torch.empty(list(vol.shape), dtype=torch.uint8, device=ctx.device)
    check(ctx.lib.nerf_grid_threshold(ctx.handle, vol.data_ptr(), vol.numel(), float(threshold), mask.data_ptr(), ctx.stream()))
    return mask


def dilate_mask(mask, steps=1):
    """``steps`` steps of svox2's ``dilate``: the OR over the 27-neighbourhood, indices clamped at the faces. ``mask`` is a
    bool or uint8 ``[X, Y, Z]`` device tensor; the result has its dtype."""
    m = _volume_arg(mask, "mask", torch.uint8)
    ctx = get_context(m.device)
    as_bool = m.dtype == torch.bool
    cur = _as_u8(m)
    reso = (C.c_int32 * 3)(*cur.shape)
    for _ in range(int(steps)):
        nxt = torch.empty_like(cur)
        check(ctx.lib.nerf_grid_dilate(ctx.handle, reso, cur.data_ptr(), nxt.data_ptr(), ctx.stream()))
        cur = nxt
    return cur.view(torch.bool) if as_bool else cur


def compact_mask(mask):
    """``(links, count)``: int32 ``[X, Y, Z]`` with the running index over the kept nodes in C order (else -1), and the number
    of kept nodes as a one-element int32 device tensor (reading it waits for the device)."""
    m = _volume_arg(mask, "mask", torch.uint8)
    ctx = get_context(m.device)
    cur = _as_u8(m)
    links = torch.empty(list(cur.shape), dtype=torch.int32, device=ctx.device)
    work = torch.empty((int(ctx.lib.nerf_grid_compact_workspace(cur.numel())),), dtype=torch.int32, device=ctx.device)
    count = torch.zeros((1,), dtype=torch.int32, device=ctx.device)
    a = GridCompactArgs()
    a.reso[:] = list(cur.shape)
    a.mask, a.links, a.block_offsets, a.count = cur.data_ptr(), links.data_ptr(), work.data_ptr(), count.data_ptr()
    a.stream = ctx.stream().value
    check(ctx.lib.nerf_grid_compact(ctx.handle, C.byref(a)))
    return links, count


def _gather(grid, axes, links, volume, rows):
    ctx = grid.ctx
    cols = 3 * grid.basis_dim
    density = torch.empty((rows, 1), dtype=torch.float32, device=ctx.device)
    sh = torch.empty((rows, cols), dtype=torch.float32, device=ctx.device)
    if rows:
        node_of_row = torch.empty((rows,), dtype=torch.int32, device=ctx.device)
        a = GridGatherArgs()
        a.reso[:] = list(links.shape)
        a.xs, a.ys, a.zs = axes[0].data_ptr(), axes[1].data_ptr(), axes[2].data_ptr()
        a.links, a.lattice_density, a.rows = links.data_ptr(), volume.data_ptr(), rows
        a.node_of_row, a.density_data, a.sh_data = node_of_row.data_ptr(), density.data_ptr(), sh.data_ptr()
        a.stream = ctx.stream().value
        check(ctx.lib.nerf_grid_gather(grid._handle(), C.byref(a)))
    return density, sh


def _check_resample_args(grid, reso, sigma_thresh, weight_thresh, dilate, cameras, weight_render_stop_thresh, max_elements):
    """Everything that can be refused is refused here, before anything is launched or changed."""
    _refuse_half(grid, "resample_grid")
    if not isinstance(grid, SparseGrid):
        raise TypeError("resample_grid needs a SparseGrid")
    reso = _reso3(reso)
    for name, v in (("sigma_thresh", sigma_thresh), ("weight_thresh", weight_thresh),
                    ("weight_render_stop_thresh", weight_render_stop_thresh)):
        if not isinstance(v, (int, float, np.floating, np.integer)) or v != v:
            raise ValueError(f"{name} = {v!r} must be a number")
    if not isinstance(dilate, (int, np.integer, bool)) or int(dilate) < 0:
        raise ValueError(f"dilate = {dilate!r} must be a non-negative int")
    if not isinstance(max_elements, (int, np.integer)) or int(max_elements) < 0:
        raise ValueError(f"max_elements = {max_elements!r} must be a non-negative int")
    if cameras is not None:
        cameras = list(cameras)
        for cam in cameras:
            if not isinstance(cam, Camera):
                raise TypeError("cameras must be a list of grid Cameras (OpenCV convention)")
            cam._to_c()      # NDC cameras and bad poses are refused now
    if grid.opt.last_sample_opaque:
        raise NotImplementedError("last_sample_opaque is not built")
    return reso, cameras


def _resample_tensors(grid, reso, sigma_thresh, weight_thresh, dilate, cameras, weight_render_stop_thresh, max_elements):
    ctx = grid.ctx
    axes = _axes_arg(lattice_axes(list(grid.links.shape), reso), reso, ctx)
    volume = lattice_density(grid, axes)
    if cameras is not None:
        source = torch.zeros(reso, dtype=torch.float32, device=ctx.device)
        for cam in cameras:
            weight_render(volume, cam, grid.radius, grid.center, 0.5, weight_render_stop_thresh, out=source)
        thresh = float(weight_thresh)
    else:
        source, thresh = volume, float(sigma_thresh)
    mask = threshold_mask(source, thresh)
    if 0 < max_elements < source.numel() and max_elements < int(torch.count_nonzero(mask)):
        # svox2's bound on the memory: the threshold rises to the max_elements-th largest value
        bounded = float(torch.topk(source.view(-1), k=int(max_elements), sorted=False).values.min())
        thresh = max(thresh, bounded)
        mask = threshold_mask(source, thresh)
    if dilate:
        mask = dilate_mask(mask, int(dilate))
    links, count = compact_mask(mask)
    rows = int(count.item())      # the one wait: the tables must be allocated
    density, sh = _gather(grid, axes, links, volume, rows)
    return links, density, sh


def resample_grid(grid, reso, sigma_thresh=5.0, weight_thresh=0.01, dilate=2, cameras=None, accelerate=True,
                  weight_render_stop_thresh=0.2, max_elements=0):
    """svox2's ``SparseGrid.resample`` as a function that returns a NEW grid of ``reso`` (an int or three) with ``grid``'s
    radius, center, basis and ``opt``; ``grid`` is untouched and still usable.

    The density of ``grid`` is sampled at every node of the new lattice. A node is kept when, with ``cameras`` (a list of
    ``Camera``), its largest rendering weight over all cameras (``weight_render`` at step 0.5 with
    ``weight_render_stop_thresh``) is ``>= weight_thresh``; without cameras, when its density is ``>= sigma_thresh``.
    ``max_elements > 0`` raises that threshold to the ``max_elements``-th largest value when more nodes would pass. The mask
    is dilated ``dilate`` times, ``links`` number the kept nodes in C order, ``density_data`` holds the sampled densities
    (the values the threshold saw) and ``sh_data`` the coefficients of ``grid`` interpolated at the kept nodes. With
    ``accelerate`` the new grid gets its skip data. A mask that keeps nothing gives a valid grid of capacity 0, which
    renders the background."""
    reso, cameras = _check_resample_args(grid, reso, sigma_thresh, weight_thresh, dilate, cameras, weight_render_stop_thresh,
                                         max_elements)
    with torch.no_grad():
        links, density, sh = _resample_tensors(grid, reso, sigma_thresh, weight_thresh, dilate, cameras,
                                               weight_render_stop_thresh, int(max_elements))
    return grid._like(links, density, sh, accelerate)
