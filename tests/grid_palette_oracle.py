"""Numpy restatement of the palette quantiser (include/nerf_mi355x.h, "Sparse voxel grid: palette-quantised colours"): the
balanced median cut of order ``bits``, the quantisation of a grid's SH table with it, and the dequantisation. Written from the
header's rule, not from the kernels: boxes are tracked as explicit lists here, the kernels compute them from (m, level, j).
A plain module (no fixtures, no pytest settings)."""
import numpy as np

HALF_MAX = 65504.0


def sort_key(x):
    """uint32 keys whose unsigned order is the order of the fp32 values, -0.0 below +0.0"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def box_sizes(m, bits):
    """sizes of the 2^bits final boxes of m members"""
    sizes = [int(m)]
    for _ in range(bits):
        sizes = [s for n in sizes for s in (n - n // 2, n // 2)]
    return np.array(sizes, np.int64)


def to_half(mean64):
    """fp64 -> fp32 -> clamp -> fp16, each to nearest even"""
    return np.clip(np.asarray(mean64, np.float64).astype(np.float32), -HALF_MAX, HALF_MAX).astype(np.float16)


def median_cut(colors, bits, return_means=False):
    """``(palette fp16 [2^bits, 3], ids uint16 [m])`` of ``colors`` fp32 ``[m, 3]``; with ``return_means`` also the fp64 means
    ``[2^bits, 3]`` and the members of every final box."""
    colors = np.ascontiguousarray(colors, np.float32).reshape(-1, 3)
    if not np.isfinite(colors).all():
        raise ValueError("non-finite colours")
    boxes = [np.arange(len(colors), dtype=np.int64)]
    for _ in range(bits):
        nxt = []
        for members in boxes:
            n = len(members)
            if n >= 2:
                c = colors[members]
                extent = (c.max(axis=0) - c.min(axis=0)).astype(np.float32)      # fp32 inputs: the difference rounds once
                axis = int(np.argmax(extent))                                    # the first of equal extents
                members = members[np.argsort(sort_key(c[:, axis]), kind="stable")]
            nxt += [members[:n - n // 2], members[n - n // 2:]]
        boxes = nxt
    ids = np.zeros(len(colors), np.uint16)
    means = np.zeros((1 << bits, 3), np.float64)
    for j, members in enumerate(boxes):
        ids[members] = j
        if len(members):
            # (from -0.0, the identity of addition; numpy's own sum starts at +0.0 and would lose the sign of a -0.0)
            means[j] = np.add.reduce(colors[members].astype(np.float64), axis=0, initial=-0.0) / len(members)
    palette = to_half(means)
    return (palette, ids, means, boxes) if return_means else (palette, ids)


def quantise_table(sh, density, basis_dim, bits, retain=0, sigma_thresh=None):
    """compression.py on a channel-major table ``sh [capacity, 3 * basis_dim]``: ``dict`` with the file's arrays -
    ``quant_colors [Q, 2^bits, 3]`` fp16, ``quant_map [Q, capacity]`` uint16, ``data_retained [retain, capacity, 3]`` fp16 - and
    ``density_data``. Rows with ``density <= sigma_thresh`` are left out of the cut and get density 0, index 0 and zero retained."""
    sh = np.asarray(sh, np.float32)
    cap, B = sh.shape[0], basis_dim
    triples = sh.reshape(cap, 3, B)
    keep = np.ones(cap, bool) if sigma_thresh is None else np.asarray(density)[:, 0] > sigma_thresh
    out_density = np.where(keep[:, None], density, 0).astype(np.float32)
    retained = np.zeros((retain, cap, 3), np.float16)
    for k in range(retain):
        retained[k][keep] = np.clip(triples[keep, :, k], -HALF_MAX, HALF_MAX).astype(np.float16)
    colors = np.zeros((B - retain, 1 << bits, 3), np.float16)
    qmap = np.zeros((B - retain, cap), np.uint16)
    for q in range(B - retain):
        colors[q], ids = median_cut(triples[keep, :, retain + q], bits)
        qmap[q][keep] = ids
    return {"quant_colors": colors, "quant_map": qmap, "data_retained": retained, "density_data": out_density}


def dequantise(quant_colors, quant_map, data_retained):
    """the fp32 table ``[capacity, 3 * basis_dim]``, channel-major, of the file's arrays"""
    retain, Q = data_retained.shape[0], quant_colors.shape[0]
    cap, B = quant_map.shape[1] if Q else data_retained.shape[1], retain + Q
    out = np.zeros((cap, 3, B), np.float32)
    for k in range(retain):
        out[:, :, k] = data_retained[k].astype(np.float32)
    for q in range(Q):
        out[:, :, retain + q] = quant_colors[q][quant_map[q].astype(np.int64)].astype(np.float32)
    return out.reshape(cap, 3 * B)
