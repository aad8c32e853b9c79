"""Floater views of a sparse voxel grid (Plenoxels): the connected components that ``compute_FDR`` labels, projected into a
camera on the GPU.

This is svox2's ``opt/util/floater_visualization.py``: per camera view, which pixels are hit by *visible* floaters, and which
object every voxel belongs to. The reference copies the labels to the host and walks every voxel in Python loops; here the
labels and the depth map stay on the device and the scans are the HIP kernels of csrc/grid_floater_kernels.hip (semantics:
include/nerf_mi355x.h, "Sparse voxel grid: floater views"). The mapping::

    floater_visualization.py                           here
    project_floaters_to_view(grid, fdr, camera, ...)   project_floaters_to_view(grid, fdr, camera, ...,
                                                                                depth_map=None, return_counts=False)
    create_floater_overlay_on_render(rgb, heatmap)     floater_overlay_on_render(rgb, heatmap)
    create_multi_object_voxel_overlay(rgb, grid, ...)  multi_object_overlay(rgb, grid, ...)   on  component_view(grid, ...)
    create_main_object_voxel_overlay(rgb, grid, ...)   main_object_overlay(rgb, grid, ...)

Deviations: every image is a device tensor (``.cpu().numpy()`` gives the reference's array); the painted disc is the fixed set
``dx^2 + dy^2 <= 5`` and nothing is subsampled at random; the overlays project with the camera's ``cx`` / ``cy`` as the heatmap
does (the reference's overlays assume the image centre); the Canny border of the red tint is a stated rule. Two quirks are
kept: a voxel is placed at ``(idx / reso) * 2 - 1`` (its corner, not ``grid2world``'s centre) and the occlusion test compares
the camera-space z with a depth along the ray. There is no CPU or PyTorch fallback. ``fdr_results`` is what ``compute_FDR``
returns or the ``FDR_``-prefixed flattening of ``compute_all_advanced_metrics``.
"""
import ctypes as C

import numpy as np
import torch

from ._lib import NERF_GRID_FLOATER_COUNTER_INTS, GridComponentViewArgs, GridFloaterHeatmapArgs, check
from .grid import NdcCamera, SparseGrid, _volume_arg
from .grid_components import component_volumes

__all__ = ["project_floaters_to_view", "component_view", "multi_object_overlay", "main_object_overlay",
           "floater_overlay_on_render", "OBJECT_COLORS", "FLOATER_COLOR", "MAIN_OBJECT_COLOR"]

# the reference's palette of create_multi_object_voxel_overlay (RGB), its floater red and its main-object green
OBJECT_COLORS = ((0, 255, 0), (0, 150, 255), (255, 200, 0), (255, 0, 255), (0, 255, 255), (255, 128, 0), (128, 0, 255),
                 (255, 255, 128), (255, 128, 255), (128, 255, 0), (0, 255, 128), (128, 128, 255))
FLOATER_COLOR = (255, 0, 0)
MAIN_OBJECT_COLOR = (0, 255, 76)


def _get(fdr_results, key):
    if fdr_results is None:
        return None
    v = fdr_results.get(key)
    return fdr_results.get("FDR_" + key) if v is None else v


def _ids(fdr_results, key):
    v = _get(fdr_results, key)
    if v is None and key == "main_component_ids":      # (the reference's older single-id form)
        one = _get(fdr_results, "main_component_id")
        v = None if one is None else [one]
    if v is None:
        return np.zeros((0,), dtype=np.int64)
    ids = np.atleast_1d(np.asarray(v.cpu() if torch.is_tensor(v) else v)).astype(np.int64).reshape(-1)
    if ids.size and ids.min() < 1:
        raise ValueError(f"{key} holds {int(ids.min())}: component ids start at 1")
    return ids


def _labels(grid, fdr_results, who):
    """The label tensor of ``fdr_results`` checked against ``grid`` (None if there is none), and the grid's handle."""
    if not isinstance(grid, SparseGrid):
        raise TypeError(f"{who} needs a SparseGrid")
    labels = _get(fdr_results, "floater_mask_3d")
    if labels is None:
        return None, None
    h = grid._handle()      # CPU tensors, wrong dtypes and shapes of the grid are refused here
    labels = _volume_arg(labels, "floater_mask_3d", torch.int32, grid.ctx)
    if tuple(labels.shape) != tuple(grid.links.shape):
        raise ValueError(f"floater_mask_3d is {tuple(labels.shape)}, the grid's links {tuple(grid.links.shape)}")
    return labels, h


def _w2c(camera):
    """12 floats: the fp64 inverse of the 4 x 4 ``c2w``, rounded to fp32, rows 0..2."""
    m = np.asarray(torch.as_tensor(camera.c2w).detach().cpu(), dtype=np.float64)
    full = np.eye(4)
    full[:3] = m[:3]
    return np.linalg.inv(full).astype(np.float32)[:3].reshape(-1).tolist()


def _fill_view(a, grid, labels, table, camera):
    a.labels, a.table, a.n_labels = labels.data_ptr(), table.data_ptr(), table.numel() - 1
    a.radius[:] = grid.radius.tolist()
    a.center[:] = grid.center.tolist()
    a.w2c[:] = _w2c(camera)
    a.stream = grid.ctx.stream().value


def _table(ctx, entries, n_labels):
    """int32 device table ``[n_labels + 1]`` from ``[(ids, value), ...]``; later entries win."""
    t = np.zeros((n_labels + 1,), dtype=np.int32)
    for ids, value in entries:
        t[ids] = value
    return torch.from_numpy(t).to(ctx.device)


def _n_labels(fdr_results, *id_lists):
    n = _get(fdr_results, "num_components")
    top = max([int(ids.max()) for ids in id_lists if ids.size] + [0])
    return max(int(n) if n is not None else 0, top)


def _depth_arg(grid, camera, depth_map):
    if depth_map is None:
        return grid.volume_render_depth_image(camera, sigma_thresh=0.0)
    if not torch.is_tensor(depth_map):
        raise TypeError("depth_map must be a tensor")
    if not depth_map.is_cuda:
        raise RuntimeError("depth_map is on the CPU: the floater views have no CPU fallback")
    if depth_map.device != grid.ctx.device:
        raise RuntimeError(f"depth_map is on {depth_map.device}, the grid on {grid.ctx.device}")
    if depth_map.dtype != torch.float32:
        raise TypeError(f"depth_map must be float32, got {depth_map.dtype}")
    hw = (int(camera.height), int(camera.width))
    if tuple(depth_map.shape) not in (hw, hw + (1,)):
        raise ValueError(f"depth_map must be {list(hw)} or {list(hw) + [1]}, got {list(depth_map.shape)}")
    return depth_map.detach().contiguous()


def _pinhole(camera):
    """The C camera; ``Camera`` refuses ``ndc_coeffs`` itself, an ``NdcCamera`` is refused here."""
    if isinstance(camera, NdcCamera):
        raise NotImplementedError("the floater views project world points through a pinhole camera: an NDC camera (NdcCamera) "
                                  "has no such view")
    return camera._to_c()


def project_floaters_to_view(grid, fdr_results, camera, render_size=None, filter_occluded=True, min_density=0.1,
                             depth_map=None, return_counts=False):
    """float32 ``[H, W]`` device tensor: how many visible floater voxels project to every pixel of ``camera``, dilated by
    3 x 3. A floater voxel counts if its density is at least ``min_density`` (when that is positive), it projects into the
    image (and into ``render_size = (H, W)`` when given) and, with ``filter_occluded``, it is not behind the rendered surface:
    ``z < depth + 0.05 or depth < 0.01``. ``depth_map``: the camera's ``[height, width]`` depth to test against; by default
    ``grid.volume_render_depth_image(camera, sigma_thresh=0.0)``. ``None`` when ``fdr_results`` has no label tensor or no
    floater id. With ``return_counts``: ``(heatmap, {"in_view": n, "dense": n, "visible": n})``, the voxels that pass the
    density filter, those of them in the image, and those of them that are visible; reading them waits for the device."""
    labels, h = _labels(grid, fdr_results, "project_floaters_to_view")
    floater_ids = _ids(fdr_results, "floater_component_ids")
    if labels is None or floater_ids.size == 0:
        return None
    ctx = grid.ctx
    cam = _pinhole(camera)
    H, W = (int(camera.height), int(camera.width)) if render_size is None else (int(render_size[0]), int(render_size[1]))
    with torch.no_grad():
        depth = _depth_arg(grid, camera, depth_map) if filter_occluded else None
        table = _table(ctx, [(floater_ids, 1)], _n_labels(fdr_results, floater_ids))
        counts = torch.empty((max(H, 0), max(W, 0)), dtype=torch.int32, device=ctx.device)
        counters = torch.empty((3 + NERF_GRID_FLOATER_COUNTER_INTS,), dtype=torch.int32, device=ctx.device)
        heatmap = torch.empty((max(H, 0), max(W, 0)), dtype=torch.float32, device=ctx.device)
        a = GridFloaterHeatmapArgs()
        _fill_view(a, grid, labels, table, camera)
        a.min_density = float(min_density)
        a.filter_occluded = 1 if filter_occluded else 0
        a.depth = depth.data_ptr() if depth is not None else None
        a.out_width, a.out_height = W, H
        a.counts, a.counters, a.heatmap = counts.data_ptr(), counters.data_ptr(), heatmap.data_ptr()
        a.counter_slots = counters[3:].data_ptr()
        check(ctx.lib.nerf_grid_floater_heatmap(h, C.byref(cam), C.byref(a)))
        if not return_counts:
            return heatmap
        dense, in_view, visible = counters[:3].cpu().tolist()
    return heatmap, {"in_view": in_view, "dense": dense, "visible": visible}


def _slots(grid, labels, h, camera, table):
    ctx = grid.ctx
    cam = _pinhole(camera)
    hw = (int(camera.height), int(camera.width))
    keys = torch.empty(hw, dtype=torch.int64, device=ctx.device)
    slots = torch.empty(hw, dtype=torch.int32, device=ctx.device)
    a = GridComponentViewArgs()
    _fill_view(a, grid, labels, table, camera)
    a.keys, a.slots = keys.data_ptr(), slots.data_ptr()
    check(ctx.lib.nerf_grid_component_view(h, C.byref(cam), C.byref(a)))
    return slots


def _component_view(grid, fdr_results, camera, show_floaters, min_viz_size, who):
    """``(slots, n_main_drawn)`` or ``(None, 0)`` without a label tensor."""
    labels, h = _labels(grid, fdr_results, who)
    if labels is None:
        return None, 0
    main_ids = _ids(fdr_results, "main_component_ids")
    floater_ids = _ids(fdr_results, "floater_component_ids")
    n = _n_labels(fdr_results, main_ids, floater_ids)
    with torch.no_grad():
        if main_ids.size and min_viz_size > 0:
            volumes = component_volumes(labels, n).cpu().numpy()      # (waits for the device)
            main_ids = main_ids[volumes[main_ids - 1] >= min_viz_size]
        entries = [(main_ids, np.arange(1, main_ids.size + 1, dtype=np.int32))]
        if show_floaters:
            entries.insert(0, (floater_ids, main_ids.size + 1))
        return _slots(grid, labels, h, camera, _table(grid.ctx, entries, n)), int(main_ids.size)


def component_view(grid, fdr_results, camera, show_floaters=True, min_viz_size=5000):
    """int32 ``[height, width]`` device tensor of slots: 0 where nothing is drawn, ``s >= 1`` for the s-th component of
    ``main_component_ids`` whose volume reaches ``min_viz_size`` (in that order), and ``n_main_drawn + 1`` for floaters when
    ``show_floaters``. Every voxel of a drawn component covers the 21 pixels ``dx^2 + dy^2 <= 5`` around its projection; a
    pixel shows the covering voxel nearest to the camera (smallest camera-space z, then smallest slot). ``None`` when
    ``fdr_results`` has no label tensor. With ``min_viz_size > 0`` the component volumes are read once, which waits for the
    device."""
    return _component_view(grid, fdr_results, camera, show_floaters, min_viz_size, "component_view")[0]


def _rgb_arg(rgb_image, camera, ctx):
    if not torch.is_tensor(rgb_image):
        raise TypeError("rgb_image must be a tensor")
    if not rgb_image.is_cuda:
        raise RuntimeError("rgb_image is on the CPU: the floater views have no CPU fallback")
    want = (int(camera.height), int(camera.width), 3)
    if tuple(rgb_image.shape) != want or rgb_image.dtype != torch.float32:
        raise ValueError(f"rgb_image must be float32 {list(want)}, got {rgb_image.dtype} {list(rgb_image.shape)}")
    return rgb_image.detach().to(ctx.device)


def _blend(rgb, colours, drawn, alpha):
    """``clip((1 - alpha) * rgb + alpha * (vis / 255), 0, 1)``: ``vis = trunc(rgb * 255)`` as uint8 with ``colours`` where ``drawn``."""
    vis = (rgb * 255).to(torch.uint8)
    vis = torch.where(drawn.unsqueeze(-1), colours, vis)
    # vis / 255 from a table of the 256 correctly rounded quotients (a division by a scalar may be a multiplication on the device)
    unit = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255.0)).to(rgb.device)
    return (rgb * (1 - alpha) + unit[vis.to(torch.int64)] * alpha).clamp(0, 1)


def multi_object_overlay(rgb_image, grid, fdr_results, camera, alpha=0.7, show_floaters=True, min_viz_size=5000):
    """float32 ``[H, W, 3]``: ``rgb_image`` blended with :func:`component_view` coloured by the reference's 12-entry palette
    (``OBJECT_COLORS[(slot - 1) % 12]``), floaters red. ``rgb_image`` itself when there is no label tensor."""
    slots, n_main = _component_view(grid, fdr_results, camera, show_floaters, min_viz_size, "multi_object_overlay")
    if slots is None:
        return rgb_image
    rgb = _rgb_arg(rgb_image, camera, grid.ctx)
    with torch.no_grad():
        palette = torch.tensor(OBJECT_COLORS, dtype=torch.uint8, device=rgb.device)
        s = slots.to(torch.int64)
        colours = palette[(s - 1).clamp_min(0) % len(OBJECT_COLORS)]
        red = torch.tensor(FLOATER_COLOR, dtype=torch.uint8, device=rgb.device)
        colours = torch.where((s == n_main + 1).unsqueeze(-1), red, colours)
        return _blend(rgb, colours, s > 0, alpha)


def main_object_overlay(rgb_image, grid, fdr_results, camera, alpha=0.7):
    """float32 ``[H, W, 3]``: ``rgb_image`` blended with the discs of every voxel of every main component, in one colour
    (``MAIN_OBJECT_COLOR``). ``rgb_image`` itself when there is no label tensor or no main component."""
    labels, h = _labels(grid, fdr_results, "main_object_overlay")
    main_ids = _ids(fdr_results, "main_component_ids")
    if labels is None or main_ids.size == 0:
        return rgb_image
    rgb = _rgb_arg(rgb_image, camera, grid.ctx)
    with torch.no_grad():
        slots = _slots(grid, labels, h, camera, _table(grid.ctx, [(main_ids, 1)], _n_labels(fdr_results, main_ids)))
        green = torch.tensor(MAIN_OBJECT_COLOR, dtype=torch.uint8, device=rgb.device).expand(rgb.shape)
        return _blend(rgb, green, slots > 0, alpha)


def floater_overlay_on_render(rgb_image, heatmap, alpha=0.9):
    """float32 ``[H, W, 3]``: the reference's red tint, ``(1 - alpha) * rgb + alpha * red * heatmap / max`` where the heatmap is
    positive, clipped to ``[0, 1]``. In place of the reference's Canny border: a masked pixel with a 4-neighbour inside the
    image and outside the mask becomes pure red. ``rgb_image`` itself when ``heatmap`` is None; unchanged values when it is all
    zero (decided on the device: nothing waits)."""
    if heatmap is None or rgb_image is None:
        return rgb_image
    if not (torch.is_tensor(rgb_image) and torch.is_tensor(heatmap) and rgb_image.is_cuda and heatmap.is_cuda):
        raise RuntimeError("rgb_image and heatmap must be device tensors: the floater views have no CPU fallback")
    if rgb_image.dim() != 3 or rgb_image.shape[2] != 3 or tuple(heatmap.shape) != tuple(rgb_image.shape[:2]):
        raise ValueError(f"rgb_image must be [H, W, 3] and heatmap [H, W], got {list(rgb_image.shape)} and {list(heatmap.shape)}")
    with torch.no_grad():
        rgb = rgb_image.detach().to(torch.float32)
        heat = heatmap.detach().to(torch.float32)
        mask = heat > 0
        norm = heat / heat.max().clamp_min(torch.finfo(torch.float32).tiny)
        red = torch.tensor([1.0, 0.0, 0.0], dtype=torch.float32, device=rgb.device)
        tint = rgb * (1 - alpha) + (norm.unsqueeze(-1) * red) * alpha
        out = torch.where(mask.unsqueeze(-1), tint, rgb)
        outside = ~mask
        edge = torch.zeros_like(mask)
        edge[1:, :] |= outside[:-1, :]
        edge[:-1, :] |= outside[1:, :]
        edge[:, 1:] |= outside[:, :-1]
        edge[:, :-1] |= outside[:, 1:]
        out = torch.where((mask & edge).unsqueeze(-1), red, out)
        return out.clamp(0, 1)
