"""Floater detection on a sparse voxel grid (Plenoxels): the connected components of the occupied nodes, on the GPU.

``compute_FDR(grid, ...)`` is the *Floater Detection Ratio* of svox2's ``opt/util/advanced_metrics.py`` with its arguments,
defaults, keys and Python types: the share of occupied voxels that sit in small disconnected components of the density
field. The reference copies the grid to the host and labels a dense array there; here occupancy, labelling and the component
volumes are the HIP kernels of csrc/grid_components_kernels.hip (semantics: include/nerf_mi355x.h, "Sparse voxel grid:
connected components"), and only the classification of the ``n`` component volumes runs on the host, in numpy. The mapping::

    advanced_metrics.py                                here
    compute_FDR(grid, ...)                             compute_FDR(grid, ...)          (labels stay on the device)
    ndimage.label(occupied, structure)                 labels, volumes = label_components(grid, threshold, ..., connectivity)
    ndimage.sum(occupied, labeled, range(1, n + 1))        "
    compute_MCQ / compute_all_advanced_metrics         the same names
    (nothing)                                          new, result = remove_floaters(grid, ...)
                                                       trainer.remove_floaters(...)    (in place)

Two deviations: ``floater_mask_3d`` is the int32 ``[X, Y, Z]`` label tensor on the device (``.cpu().numpy()`` gives the
reference's array), and ``verbose`` prints other text. There is no CPU or PyTorch fallback and no scipy. One labelling waits
for the device once, to read the component count.
"""
import ctypes as C

import numpy as np
import torch

from ._lib import GridCopyRowsArgs, GridLabelArgs, GridOccupancyArgs, check
from .grid import SparseGrid, _as_u8, _refuse_half, _reso3, _volume_arg
from .grid_resample import compact_mask
from .host import get_context

__all__ = ["label_components", "classify_components", "compute_FDR", "compute_MCQ", "compute_all_advanced_metrics",
           "remove_floaters"]


def _check_connectivity(connectivity):
    if isinstance(connectivity, bool) or connectivity not in (6, 18, 26):
        raise ValueError(f"Invalid connectivity: {connectivity}. Must be 6, 18, or 26.")
    return int(connectivity)


def _check_grid(grid, who):
    if not isinstance(grid, SparseGrid):
        raise TypeError(f"{who} needs a SparseGrid")
    _reso3(list(grid.links.shape), "links.shape")
    return grid._handle()      # CPU tensors, wrong dtypes and shapes are refused here


def occupancy(grid, threshold=0.01, use_density_threshold=True):
    """uint8 ``[X, Y, Z]``: 1 where a node is kept (``links >= 0``) and, when ``use_density_threshold and threshold > 0``,
    its density is ``> float32(threshold)``."""
    h = _check_grid(grid, "occupancy")
    ctx = grid.ctx
    occ = torch.empty(list(grid.links.shape), dtype=torch.uint8, device=ctx.device)
    a = GridOccupancyArgs()
    a.use_density = 1 if (use_density_threshold and threshold > 0) else 0
    a.threshold = float(threshold) if a.use_density else 0.0
    a.occupied, a.stream = occ.data_ptr(), ctx.stream().value
    check(ctx.lib.nerf_grid_components_occupancy(h, C.byref(a)))
    return occ


def label_mask(occupied, connectivity=26):
    """``(labels, count)`` of a uint8 / bool ``[X, Y, Z]`` device mask: int32 labels 1..count in increasing order of the
    components' smallest C-order index, 0 where the mask is 0. Waits for the device once, for ``count``."""
    connectivity = _check_connectivity(connectivity)
    m = _volume_arg(occupied, "occupied", torch.uint8)
    ctx = get_context(m.device)
    occ = _as_u8(m)
    dev = ctx.device
    labels = torch.empty(list(occ.shape), dtype=torch.int32, device=dev)
    parent = torch.empty(list(occ.shape), dtype=torch.int32, device=dev)
    work = torch.empty((int(ctx.lib.nerf_grid_components_workspace(occ.numel())),), dtype=torch.int32, device=dev)
    status = torch.empty((2,), dtype=torch.int32, device=dev)
    a = GridLabelArgs()
    a.reso[:] = list(occ.shape)
    a.connectivity = connectivity
    a.occupied, a.parent, a.block_offsets = occ.data_ptr(), parent.data_ptr(), work.data_ptr()
    a.labels, a.status, a.stream = labels.data_ptr(), status.data_ptr(), ctx.stream().value
    check(ctx.lib.nerf_grid_components_label(ctx.handle, C.byref(a)))
    count = C.c_int64(0)
    check(ctx.lib.nerf_grid_components_finish(ctx.handle, status.data_ptr(), C.byref(count), ctx.stream()))
    return labels, int(count.value)


def component_volumes(labels, count):
    """int64 ``[count]`` device tensor: the number of nodes of every label 1..count."""
    ctx = get_context(labels.device)
    vol = torch.empty((count,), dtype=torch.int32, device=ctx.device)
    check(ctx.lib.nerf_grid_components_volumes(ctx.handle, labels.data_ptr(), labels.numel(), count, vol.data_ptr(), ctx.stream()))
    return vol.to(torch.int64)


def label_components(grid, threshold=0.01, use_density_threshold=True, connectivity=26):
    """``(labels, volumes)``: the connected components (6, 18 or 26 neighbours, no wrap-around) of the occupied nodes of
    ``grid``. ``labels`` is an int32 ``[X, Y, Z]`` device tensor, 0 where a node is not occupied, else the component's number
    1..n in increasing order of its smallest C-order index (``scipy.ndimage.label``'s numbering); ``volumes`` an int64 ``[n]``
    device tensor with the node count of every component."""
    connectivity = _check_connectivity(connectivity)
    occ = occupancy(grid, threshold, use_density_threshold)
    labels, count = label_mask(occ, connectivity)
    return labels, component_volumes(labels, count)


def classify_components(volumes, min_object_size=1000, size_gap_ratio=0.2, use_adaptive=True):
    """``(floater, num_main_objects, detection_method)`` from the component volumes alone, the reference's rule: simple mode
    calls every component below ``min_object_size`` a floater; adaptive mode does the same and then walks the remaining ones
    in descending size to the first whose size is less than ``size_gap_ratio`` times its predecessor's - that one and all
    after it are floaters too. ``floater`` is a bool array in component order."""
    vol = np.asarray(volumes, dtype=np.float64)
    small = vol < min_object_size
    if not use_adaptive:
        n_main = np.sum(~small)
        return small, n_main, f"simple_threshold (min_size={min_object_size}, {n_main} objects >= threshold)"
    floater = small.copy()
    big_ids = np.flatnonzero(~small)
    big_ids = big_ids[np.argsort(-vol[big_ids], kind="stable")]
    big = vol[big_ids]
    if big.size > 1:
        ratios = big[1:] / big[:-1]
        gaps = np.flatnonzero(ratios < size_gap_ratio)
        if gaps.size:
            n_main = gaps[0] + 1
            floater[big_ids[n_main:]] = True
            method = f"adaptive_gap (gap after {n_main} objects, ratio={ratios[gaps[0]]:.3f})"
        else:
            n_main = big.size
            method = f"adaptive_nogap ({n_main} main objects, no clear gap)"
    else:
        n_main = big.size
        method = f"adaptive_single ({n_main} main objects)"
    n_small = small.sum()
    if n_small > 0:
        method += f" + {n_small} below min_size"
    return floater, n_main, method


def fdr_from_volumes(volumes, reso, connectivity, min_object_size=1000, size_gap_ratio=0.2, use_adaptive=True):
    """The reference's result dict (without ``floater_mask_3d``) from the component volumes of a lattice ``reso``."""
    if len(volumes) == 0:
        return {"FDR": 0.0, "num_floaters": 0, "num_components": 0, "main_volume": 0, "floater_volume": 0, "total_volume": 0,
                "sparsity": 1.0, "largest_floater": 0, "mean_floater_size": 0.0}
    vol = np.asarray(volumes, dtype=np.float64)      # (the reference's volumes are ndimage.sum's doubles)
    floater, n_main, method = classify_components(vol, min_object_size, size_gap_ratio, use_adaptive)
    fl, main = vol[floater], vol[~floater]
    total = np.sum(vol)
    floater_volume = np.sum(fl)
    return {
        "FDR": float(floater_volume / total if total > 0 else 0.0),
        "num_floaters": int(np.sum(floater)),
        "num_components": int(len(vol)),
        "num_main_objects": int(n_main),
        "main_volume": int(np.sum(main) if len(main) else 0),
        "largest_main_volume": int(np.max(main) if len(main) else 0),
        "floater_volume": int(floater_volume),
        "total_volume": int(total),
        "sparsity": float(1.0 - (total / int(np.prod(reso)))),
        "largest_floater": int(np.max(fl) if len(fl) else 0),
        "mean_floater_size": float(np.mean(fl) if len(fl) else 0.0),
        "detection_method": method,
        "connectivity": connectivity,
        "floater_component_ids": np.where(floater)[0] + 1,
        "main_component_ids": np.where(~floater)[0] + 1,
    }


def compute_FDR(grid, threshold=0.01, main_object_threshold=0.05, use_density_threshold=True, max_resolution=None,
                min_object_size=1000, size_gap_ratio=0.2, use_adaptive=True, connectivity=26, verbose=False):
    """The Floater Detection Ratio of ``grid``: ``floater_volume / total_volume`` over the connected components of its
    occupied nodes, with the reference's keys (``FDR``, ``num_floaters``, ``num_components``, ``num_main_objects``,
    ``main_volume``, ``largest_main_volume``, ``floater_volume``, ``total_volume``, ``sparsity``, ``largest_floater``,
    ``mean_floater_size``, ``detection_method``, ``connectivity``, ``floater_mask_3d``, ``floater_component_ids``,
    ``main_component_ids``; the nine-key form for an empty occupancy). ``floater_mask_3d`` is the int32 label tensor on the
    device. ``main_object_threshold`` and ``max_resolution`` are accepted and unused, as in the reference."""
    labels, volumes = label_components(grid, threshold, use_density_threshold, connectivity)
    out = fdr_from_volumes(volumes.cpu().numpy(), list(grid.links.shape), connectivity, min_object_size, size_gap_ratio,
                           use_adaptive)
    if out["num_components"]:
        ids = (out.pop("floater_component_ids"), out.pop("main_component_ids"))
        out["floater_mask_3d"] = labels
        out["floater_component_ids"], out["main_component_ids"] = ids
    if verbose:
        print(f"    FDR {out['FDR']:.2%}: {out['num_floaters']} floaters of {out['num_components']} components, "
              f"{out.get('detection_method', 'empty')}")
    return out


def compute_MCQ(psnr, peak_gpu_memory_mb):
    """Memory Cost per Quality: peak GPU memory in GB per dB of PSNR (0 when ``psnr <= 0``)."""
    peak_gpu_gb = peak_gpu_memory_mb / 1024.0
    mcq = peak_gpu_gb / psnr if psnr > 0 else 0.0
    return {"MCQ": mcq, "peak_gpu_gb": peak_gpu_gb, "peak_gpu_mb": peak_gpu_memory_mb, "psnr": psnr, "memory_per_db": mcq}


def compute_all_advanced_metrics(grid, psnr, use_fp16=False, compute_fdr=True, fdr_threshold=0.01,
                                 fdr_main_object_threshold=0.1, fdr_min_object_size=1000, fdr_size_gap_ratio=0.2,
                                 fdr_use_adaptive=True, fdr_connectivity=26, peak_gpu_memory_mb=None, verbose=True):
    """MCQ (when ``peak_gpu_memory_mb`` is given) and FDR (when ``compute_fdr``) in one dict: every key of either prefixed
    ``MCQ_`` / ``FDR_``, and ``MCQ`` / ``FDR`` themselves at the top level."""
    results = {}
    if peak_gpu_memory_mb is not None:
        mcq = compute_MCQ(psnr, peak_gpu_memory_mb)
        results.update({f"MCQ_{k}": v for k, v in mcq.items()})
        results["MCQ"] = mcq["MCQ"]
    if compute_fdr:
        fdr = compute_FDR(grid, threshold=fdr_threshold, main_object_threshold=fdr_main_object_threshold,
                          min_object_size=fdr_min_object_size, size_gap_ratio=fdr_size_gap_ratio, use_adaptive=fdr_use_adaptive,
                          connectivity=fdr_connectivity, verbose=verbose)
        results.update({f"FDR_{k}": v for k, v in fdr.items()})
        results["FDR"] = fdr["FDR"]
    return results


def _copy_rows(grid, new_links, rows):
    ctx = grid.ctx
    cols = int(grid.sh_data.shape[1])
    density = torch.empty((rows, 1), dtype=torch.float32, device=ctx.device)
    sh = torch.empty((rows, cols), dtype=torch.float32, device=ctx.device)
    if rows:
        src = torch.empty((rows,), dtype=torch.int32, device=ctx.device)
        a = GridCopyRowsArgs()
        a.reso[:] = list(new_links.shape)
        a.cols = cols
        a.old_links, a.new_links = grid.links.data_ptr(), new_links.data_ptr()
        a.old_rows, a.new_rows = int(grid.density_data.shape[0]), rows
        a.old_density, a.old_sh = grid.density_data.data_ptr(), grid.sh_data.data_ptr()
        a.src_row, a.density, a.sh = src.data_ptr(), density.data_ptr(), sh.data_ptr()
        a.stream = ctx.stream().value
        check(ctx.lib.nerf_grid_copy_rows(ctx.handle, C.byref(a)))
    return density, sh


def _without_floaters(grid, fdr_kwargs):
    """``(links, density_data, sh_data, result)`` of ``grid`` without the components ``compute_FDR`` calls floaters."""
    _refuse_half(grid, "remove_floaters")
    _check_grid(grid, "remove_floaters")
    result = compute_FDR(grid, **fdr_kwargs)      # every argument is checked in here, before anything is made
    ctx = grid.ctx
    n = grid.links.numel()
    count = result["num_components"]
    if count:
        labels = result["floater_mask_3d"]
        table = np.zeros((count,), dtype=np.uint8)
        table[result["floater_component_ids"] - 1] = 1
        floater = torch.from_numpy(table).to(ctx.device)
    else:      # nothing is occupied: every kept node stays
        labels = torch.zeros(list(grid.links.shape), dtype=torch.int32, device=ctx.device)
        floater = None
    mask = torch.empty(list(grid.links.shape), dtype=torch.uint8, device=ctx.device)
    check(ctx.lib.nerf_grid_components_keep(ctx.handle, grid.links.data_ptr(), labels.data_ptr(), n,
                                            floater.data_ptr() if count else None, count, mask.data_ptr(), ctx.stream()))
    links, kept = compact_mask(mask)
    rows = int(kept.item())      # the tables must be allocated
    density, sh = _copy_rows(grid, links, rows)
    return links, density, sh, result


def remove_floaters(grid, accelerate=True, **fdr_kwargs):
    """``(new_grid, result)``: ``result = compute_FDR(grid, **fdr_kwargs)`` and a NEW grid on the same lattice (radius,
    center, basis and ``opt`` of ``grid``) that has lost the nodes whose component ``result`` calls a floater. Every other
    kept node stays, those below the density threshold included; ``links`` number the kept nodes in C order and the rows of
    ``density_data`` / ``sh_data`` are copied bit for bit. ``grid`` is untouched. With ``accelerate`` the new grid gets its
    skip data."""
    with torch.no_grad():
        links, density, sh, result = _without_floaters(grid, fdr_kwargs)
    return grid._like(links, density, sh, accelerate), result
