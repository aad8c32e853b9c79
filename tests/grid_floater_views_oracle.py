"""numpy restatement of the sparse voxel grid's floater views (include/nerf_mi355x.h, "Sparse voxel grid: floater views"):
what csrc/grid_floater_kernels.hip computes, in fp32 with every operation a separate rounding, vectorised with ``np.add.at``
and ``np.minimum.at``. A test oracle (not part of the package). Grids are the dicts of grid_oracle (``links``,
``density_data``, ``radius``, ``center``); a camera is a dict ``c2w`` ([3, 4] or [4, 4]), ``fx``, ``fy``, ``cx``, ``cy``,
``width``, ``height``.

Every entry point also reports which candidate nodes are *ambiguous*: those at which a difference of a few ulp between a
GEMM's summation order, an fp32 and an fp64 matrix inverse and the order stated in the header could change the result.
A candidate node (one with a non-zero table entry) is ambiguous if
    x or y lies within 1e-3 px of an integer (or is not finite),
    q2 lies within 1e-3 of 0,
    q2 lies within 1e-4 of d + 0.05, or d within 1e-4 of 0.01 (where the depth is read),
    rho lies within 1e-6 of min_density (where the density is read).
The margins are conditions for a comparison to be exact, not tolerances: the tests assert that no node is ambiguous.
"""
import numpy as np

F = np.float32

OBJECT_COLORS = np.array([[0, 255, 0], [0, 150, 255], [255, 200, 0], [255, 0, 255], [0, 255, 255], [255, 128, 0], [128, 0, 255],
                          [255, 255, 128], [255, 128, 255], [128, 255, 0], [0, 255, 128], [128, 128, 255]], dtype=np.uint8)
FLOATER_COLOR = np.array([255, 0, 0], dtype=np.uint8)
MAIN_OBJECT_COLOR = np.array([0, 255, 76], dtype=np.uint8)
# the 21 offsets (dx, dy) of the disc dx^2 + dy^2 <= 5
DISC = [(dx, dy) for dy in range(-2, 3) for dx in range(-2, 3) if dx * dx + dy * dy <= 5]


def w2c_of(c2w):
    """[3, 4] fp32: the fp64 inverse of the 4 x 4 ``c2w``, rounded to fp32."""
    full = np.eye(4)
    full[:3] = np.asarray(c2w, dtype=np.float64)[:3]
    return np.linalg.inv(full).astype(F)[:3]


def project(grid, cam, idx):
    """``(q2, x, y, valid, xi, yi)`` of the nodes ``idx [N, 3]``: the header's projection, operation by operation."""
    shape = np.asarray(grid["links"].shape)
    radius, center = np.asarray(grid["radius"], dtype=F), np.asarray(grid["center"], dtype=F)
    m = w2c_of(cam["c2w"])
    with np.errstate(all="ignore"):
        p = ((idx.astype(F) / shape.astype(F)) * F(2) - F(1)).astype(F)
        p = (p * radius + center).astype(F)
        q = [(((m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1]).astype(F) + m[r, 2] * p[:, 2]).astype(F) + m[r, 3]).astype(F)
             for r in range(3)]
        x = ((q[0] / q[2]) * F(cam["fx"]) + F(cam["cx"])).astype(F)
        y = ((q[1] / q[2]) * F(cam["fy"]) + F(cam["cy"])).astype(F)
        valid = (q[2] > 0) & (x >= 0) & (x < F(cam["width"])) & (y >= 0) & (y < F(cam["height"]))
    xi = np.where(valid, x, 0).astype(np.int64)
    yi = np.where(valid, y, 0).astype(np.int64)
    return q[2], x, y, valid, xi, yi


def _near_integer(v, margin):
    with np.errstate(all="ignore"):
        return ~np.isfinite(v) | (np.abs(v - np.rint(v)) <= margin)


def _geometry_ambiguous(q2, x, y):
    return _near_integer(x, 1e-3) | _near_integer(y, 1e-3) | ~(np.abs(q2) > 1e-3)


def _table(ids, n_labels, value=1):
    t = np.zeros(n_labels + 1, dtype=np.int32)
    t[np.asarray(ids, dtype=np.int64)] = value
    return t


def _entries(labels, table):
    """table[label], 0 for labels outside [1, n_labels]"""
    n = len(table) - 1
    ok = (labels > 0) & (labels <= n)
    return np.where(ok, table[np.where(ok, labels, 0)], 0)


def heatmap(grid, labels, floater_ids, cam, depth=None, render_size=None, filter_occluded=True, min_density=0.1, n_labels=None):
    """``(heatmap [H, W] fp32, counts [H, W] int32 before the dilation, {"dense", "in_view", "visible"}, ambiguous)``;
    ``ambiguous`` is a bool per candidate node (floater nodes in C order). ``depth``: the camera's [height, width] map."""
    n_labels = int(max(np.max(floater_ids), labels.max())) if n_labels is None else n_labels
    cand = np.argwhere(_entries(labels, _table(floater_ids, n_labels)) != 0)
    H, W = (cam["height"], cam["width"]) if render_size is None else render_size
    links, density = grid["links"], np.asarray(grid["density_data"], dtype=F).reshape(-1)
    amb = np.zeros(len(cand), dtype=bool)
    lk = links[cand[:, 0], cand[:, 1], cand[:, 2]].astype(np.int64)
    kept = (lk >= 0) & (lk < len(density))
    rho = np.where(kept, density[np.where(kept, lk, 0)], F(0)).astype(F)
    dense = np.ones(len(cand), dtype=bool)
    if min_density > 0:
        dense = rho >= F(min_density)
        amb |= np.abs(rho.astype(np.float64) - float(F(min_density))) <= 1e-6
    q2, x, y, valid, xi, yi = project(grid, cam, cand)
    amb |= _geometry_ambiguous(q2, x, y)
    in_view = dense & valid & (xi < W) & (yi < H)
    visible = in_view.copy()
    if filter_occluded:
        d = np.asarray(depth, dtype=F).reshape(cam["height"], cam["width"])[yi, xi]
        visible = in_view & ((q2 < (d + F(0.05)).astype(F)) | (d < F(0.01)))
        dd = d.astype(np.float64)
        amb |= valid & ((np.abs(q2.astype(np.float64) - (dd + 0.05)) <= 1e-4) | (np.abs(dd - 0.01) <= 1e-4))
    counts = np.zeros((H, W), dtype=np.int32)
    np.add.at(counts, (yi[visible], xi[visible]), 1)
    out = counts.copy()
    if counts.max() > 0:      # the 3 x 3 maximum over the in-image neighbours
        pad = np.zeros((H + 2, W + 2), dtype=np.int32)
        pad[1:-1, 1:-1] = counts
        out = np.max([pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)
    n = {"dense": int(dense.sum()), "in_view": int(in_view.sum()), "visible": int(visible.sum())}
    return out.astype(F), counts, n, amb


def slot_table(labels, main_ids, floater_ids, show_floaters=True, min_viz_size=5000, n_labels=None):
    """``(table [n_labels + 1], n_main_drawn)``: the slots of component_view."""
    main_ids, floater_ids = np.asarray(main_ids, dtype=np.int64), np.asarray(floater_ids, dtype=np.int64)
    n_labels = int(max([labels.max()] + main_ids.tolist() + floater_ids.tolist())) if n_labels is None else n_labels
    volumes = np.bincount(labels[(labels > 0) & (labels <= n_labels)].reshape(-1), minlength=n_labels + 1)
    drawn = main_ids[volumes[main_ids] >= min_viz_size] if min_viz_size > 0 else main_ids
    table = np.zeros(n_labels + 1, dtype=np.int32)
    if show_floaters:
        table[floater_ids] = len(drawn) + 1
    table[drawn] = np.arange(1, len(drawn) + 1)
    return table, len(drawn)


def component_view(grid, labels, table, cam):
    """``(slots [height, width] int32, ambiguous per candidate node, ties)``: ``ties`` counts the pixels at which two
    different slots meet at the smallest q2."""
    cand = np.argwhere(_entries(labels, table) != 0)
    slot = _entries(labels, table)[cand[:, 0], cand[:, 1], cand[:, 2]].astype(np.uint64)
    q2, x, y, valid, xi, yi = project(grid, cam, cand)
    amb = _geometry_ambiguous(q2, x, y)
    H, W = cam["height"], cam["width"]
    key = (q2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | slot
    full = np.uint64(0xFFFFFFFFFFFFFFFF)
    keys = np.full(H * W, full, dtype=np.uint64)
    zmax_slot = np.zeros(H * W, dtype=np.uint64)
    cover = []
    for dx, dy in DISC:
        xx, yy = xi + dx, yi + dy
        ok = valid & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        cover.append((yy[ok] * W + xx[ok], key[ok]))
        np.minimum.at(keys, cover[-1][0], cover[-1][1])
    slots = np.where(keys == full, 0, keys & np.uint64(0xFFFFFFFF)).astype(np.int32).reshape(H, W)
    # ties: a covering node with the winning q2 and another slot
    for pix, k in cover:
        same_z = (k >> np.uint64(32)) == (keys[pix] >> np.uint64(32))
        np.maximum.at(zmax_slot, pix[same_z], k[same_z] & np.uint64(0xFFFFFFFF))
    ties = int(np.sum((keys != full) & (zmax_slot != (keys & np.uint64(0xFFFFFFFF)))))
    return slots, amb, ties


def blend(rgb, colours, drawn, alpha):
    """``clip((1 - alpha) * rgb + alpha * (vis / 255), 0, 1)`` in fp32, ``vis = trunc(rgb * 255)`` as uint8 with ``colours``
    where ``drawn``; ``1 - alpha`` is formed in double and rounded once."""
    rgb = np.asarray(rgb, dtype=F)
    vis = (rgb * F(255)).astype(np.uint8)
    vis = np.where(drawn[..., None], colours, vis)
    out = (F(1 - alpha) * rgb + F(alpha) * (vis.astype(F) / F(255.0))).astype(F)
    return np.clip(out, 0, 1)


def multi_object_overlay(rgb, slots, n_main_drawn, alpha=0.7, bgr=False):
    """``bgr``: the colours with channels reversed, as the reference paints them (it hands OpenCV BGR tuples for an RGB image)."""
    colours = OBJECT_COLORS[(np.maximum(slots, 1) - 1) % len(OBJECT_COLORS)]
    colours = np.where((slots == n_main_drawn + 1)[..., None], FLOATER_COLOR, colours)
    return blend(rgb, colours[..., ::-1] if bgr else colours, slots > 0, alpha)


def main_object_overlay(rgb, slots, alpha=0.7, bgr=False):
    colour = MAIN_OBJECT_COLOR[::-1] if bgr else MAIN_OBJECT_COLOR
    return blend(rgb, np.broadcast_to(colour, slots.shape + (3,)), slots > 0, alpha)


def floater_overlay_on_render(rgb, heat, alpha=0.9):
    """The red tint and the border rule (a masked pixel with a 4-neighbour inside the image and outside the mask is red)."""
    rgb, heat = np.asarray(rgb, dtype=F), np.asarray(heat, dtype=F)
    if not heat.max() > 0:
        return rgb.copy()
    mask = heat > 0
    norm = (heat / heat.max()).astype(F)
    red = np.array([1, 0, 0], dtype=F)
    tint = (F(1 - alpha) * rgb + F(alpha) * (norm[..., None] * red)).astype(F)
    out = np.where(mask[..., None], tint, rgb)
    outside = ~mask
    edge = np.zeros_like(mask)
    edge[1:, :] |= outside[:-1, :]
    edge[:-1, :] |= outside[1:, :]
    edge[:, 1:] |= outside[:, :-1]
    edge[:, :-1] |= outside[:, 1:]
    out = np.where((mask & edge)[..., None], red, out)
    return np.clip(out, 0, 1).astype(F)
