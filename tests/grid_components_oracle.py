"""Numpy restatement of the sparse voxel grid's connected components and of the Floater Detection Ratio built on them
(include/nerf_mi355x.h, "Sparse voxel grid: connected components"; svox2 opt/util/advanced_metrics.py compute_FDR).

No scipy and nothing of the product: the labelling is a union-find of its own over the list of neighbour pairs (minimum
propagation with pointer jumping, vectorised), the classification a plain loop over the sorted volumes. Used by the CPU tests
against the reference's recorded results (tests/golden/grid_components.npz) and by the GPU tests against the kernels.
"""
import numpy as np

SCALAR_KEYS = ("FDR", "num_floaters", "num_components", "num_main_objects", "main_volume", "largest_main_volume",
               "floater_volume", "total_volume", "sparsity", "largest_floater", "mean_floater_size", "detection_method",
               "connectivity")
EMPTY_KEYS = ("FDR", "num_floaters", "num_components", "main_volume", "floater_volume", "total_volume", "sparsity",
              "largest_floater", "mean_floater_size")
ARRAY_KEYS = ("floater_mask_3d", "floater_component_ids", "main_component_ids")


def occupancy(links, density_data, threshold=0.01, use_density_threshold=True):
    """bool [X, Y, Z]: kept (any negative link is empty) and, when thresholding, density > float32(threshold) in fp32."""
    kept = links >= 0
    if not (use_density_threshold and threshold > 0):
        return kept
    dens = np.zeros(links.shape, dtype=np.float32)
    dens[kept] = np.asarray(density_data, dtype=np.float32)[links[kept], 0]
    with np.errstate(invalid="ignore"):
        return kept & (dens > np.float32(threshold))


def neighbour_offsets(connectivity):
    """The half of the neighbourhood that comes before a node in C order."""
    if connectivity not in (6, 18, 26):
        raise ValueError(f"Invalid connectivity: {connectivity}. Must be 6, 18, or 26.")
    most = {6: 1, 18: 2, 26: 3}[connectivity]
    out = []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                if (dx, dy, dz) < (0, 0, 0) and abs(dx) + abs(dy) + abs(dz) <= most:
                    out.append((dx, dy, dz))
    return out


def label(occupied, connectivity=26):
    """(labels int32 [X, Y, Z], n): components numbered 1..n in increasing order of their smallest flat C-order index."""
    occ = np.asarray(occupied).astype(bool)
    sx, sy, sz = occ.shape
    flat = np.arange(occ.size, dtype=np.int64).reshape(occ.shape)
    pairs_a, pairs_b = [], []
    for dx, dy, dz in neighbour_offsets(connectivity):
        # nodes [lo, hi) per axis have the neighbour at + d inside the lattice
        sl_me = tuple(slice(max(0, -d), s - max(0, d)) for d, s in zip((dx, dy, dz), (sx, sy, sz)))
        sl_nb = tuple(slice(max(0, d), s - max(0, -d)) for d, s in zip((dx, dy, dz), (sx, sy, sz)))
        both = occ[sl_me] & occ[sl_nb]
        pairs_a.append(flat[sl_me][both])
        pairs_b.append(flat[sl_nb][both])
    a = np.concatenate(pairs_a) if pairs_a else np.zeros(0, np.int64)
    b = np.concatenate(pairs_b) if pairs_b else np.zeros(0, np.int64)
    parent = np.arange(occ.size, dtype=np.int64)
    while True:
        ra, rb = parent[a], parent[b]
        low = np.minimum(ra, rb)
        if np.array_equal(ra, rb):
            break
        np.minimum.at(parent, ra, low)
        np.minimum.at(parent, rb, low)
        while True:      # pointer jumping: every node to the root of its tree
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent = nxt
    roots = np.flatnonzero(occ.reshape(-1) & (parent == np.arange(occ.size)))      # ascending: the numbering
    number = np.zeros(occ.size, dtype=np.int32)
    number[roots] = np.arange(1, roots.size + 1, dtype=np.int32)
    labels = np.where(occ.reshape(-1), number[parent], 0).astype(np.int32).reshape(occ.shape)
    return labels, int(roots.size)


def volumes(labels, n):
    return np.bincount(labels.reshape(-1), minlength=n + 1)[1:].astype(np.int64)


def classify(vol, min_object_size=1000, size_gap_ratio=0.2, use_adaptive=True):
    """(floater bool [n], num_main_objects, detection_method) from the volumes alone."""
    n = len(vol)
    floater = [float(v) < min_object_size for v in vol]
    n_small = sum(floater)
    if not use_adaptive:
        n_main = n - n_small
        return np.array(floater, dtype=bool), n_main, f"simple_threshold (min_size={min_object_size}, {n_main} objects >= threshold)"
    order = sorted((k for k in range(n) if not floater[k]), key=lambda k: -float(vol[k]))      # descending, ties in any order
    if len(order) > 1:
        cut = None
        for pos in range(1, len(order)):
            ratio = np.float64(vol[order[pos]]) / np.float64(vol[order[pos - 1]])
            if ratio < size_gap_ratio:
                cut = pos
                break
        if cut is not None:
            for k in order[cut:]:
                floater[k] = True
            n_main = cut
            method = f"adaptive_gap (gap after {n_main} objects, ratio={ratio:.3f})"
        else:
            n_main = len(order)
            method = f"adaptive_nogap ({n_main} main objects, no clear gap)"
    else:
        n_main = len(order)
        method = f"adaptive_single ({n_main} main objects)"
    if n_small > 0:
        method += f" + {n_small} below min_size"
    return np.array(floater, dtype=bool), n_main, method


def compute_fdr(links, density_data, threshold=0.01, main_object_threshold=0.05, use_density_threshold=True, max_resolution=None,
                min_object_size=1000, size_gap_ratio=0.2, use_adaptive=True, connectivity=26):
    """The reference's dict; floater_mask_3d is the int32 label array."""
    occ = occupancy(links, density_data, threshold, use_density_threshold)
    labels, n = label(occ, connectivity)
    if n == 0:
        return {"FDR": 0.0, "num_floaters": 0, "num_components": 0, "main_volume": 0, "floater_volume": 0, "total_volume": 0,
                "sparsity": 1.0, "largest_floater": 0, "mean_floater_size": 0.0}
    vol = volumes(labels, n)
    floater, n_main, method = classify(vol, min_object_size, size_gap_ratio, use_adaptive)
    fl, main = vol[floater], vol[~floater]
    total = int(vol.sum())
    return {
        "FDR": float(np.float64(int(fl.sum())) / np.float64(total)),
        "num_floaters": int(floater.sum()),
        "num_components": n,
        "num_main_objects": int(n_main),
        "main_volume": int(main.sum()),
        "largest_main_volume": int(main.max()) if main.size else 0,
        "floater_volume": int(fl.sum()),
        "total_volume": total,
        "sparsity": float(1.0 - np.float64(total) / np.float64(int(np.prod(links.shape)))),
        "largest_floater": int(fl.max()) if fl.size else 0,
        "mean_floater_size": float(np.float64(int(fl.sum())) / np.float64(fl.size)) if fl.size else 0.0,
        "detection_method": method,
        "connectivity": connectivity,
        "floater_mask_3d": labels,
        "floater_component_ids": (np.flatnonzero(floater) + 1).astype(np.int64),
        "main_component_ids": (np.flatnonzero(~floater) + 1).astype(np.int64),
    }


def remove_floaters(links, density_data, sh_data, result):
    """(links, density_data, sh_data) without the floater components of `result`: the running index in C order, rows copied."""
    keep = links >= 0
    if result["num_components"]:
        keep &= ~np.isin(result["floater_mask_3d"], result["floater_component_ids"])
    new = np.full(links.shape, -1, dtype=np.int32)
    new[keep] = np.arange(int(keep.sum()), dtype=np.int32)
    rows = links[keep]
    return new, density_data[rows], sh_data[rows]


# ---- the fixture ----------------------------------------------------------------------------------------------------------
def fixture_cases(z):
    """[(case, grid name, kwargs)] of tests/golden/grid_components.npz."""
    out = []
    for k, case in enumerate(z["cases"]):
        kw = dict(threshold=float(z["threshold"][k]), use_density_threshold=bool(z["use_density_threshold"][k]),
                  min_object_size=int(z["min_object_size"][k]), size_gap_ratio=float(z["size_gap_ratio"][k]),
                  use_adaptive=bool(z["use_adaptive"][k]), connectivity=int(z["connectivity"][k]))
        out.append((str(case), str(z["grids"][k]), kw))
    return out


def fixture_result(z, case):
    """The reference's recorded dict of a case, with its Python types."""
    keys = [str(k) for k in z[f"{case}_keys"]]
    out = {}
    for k in keys:
        v = z[f"{case}_{k}"]
        if k in ARRAY_KEYS:
            out[k] = v
        elif v.dtype.kind == "U":
            out[k] = str(v)
        elif v.dtype.kind == "f":
            out[k] = float(v)
        else:
            out[k] = int(v)
    return out


def assert_same_result(got, want, who):
    """Every key, every value with ==, floats included; labels and ids entry by entry."""
    assert list(got.keys()) == list(want.keys()), (who, list(got.keys()), list(want.keys()))
    for k, w in want.items():
        g = got[k]
        if k in ARRAY_KEYS:
            g = np.asarray(g)
            assert g.shape == w.shape and np.array_equal(g, w), (who, k)
            if k != "floater_mask_3d":
                assert g.dtype == np.int64, (who, k, g.dtype)
        else:
            assert type(g) is type(w) and g == w, (who, k, g, w)
