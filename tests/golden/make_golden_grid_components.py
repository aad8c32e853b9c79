"""Writes tests/golden/grid_components.npz: what the reference's ``compute_FDR`` makes of a few synthetic grids.

    NERF_REFERENCE_SVOX2=/path/to/reference/svox2 python tests/golden/make_golden_grid_components.py

Runs on the CPU with scipy (the reference labels with ``scipy.ndimage.label``). The reference's
``opt/util/advanced_metrics.py`` is imported from the checkout, nothing of it is copied: the fixture holds arrays only. Its
``compute_FDR`` reads ``grid.links`` and ``grid.density_data`` and nothing else, so the grids are duck-typed objects around two
CPU tensors. Stored: per grid ``links`` (int32, with negative values other than -1 among the empty nodes) and ``density_data``
(rows in permuted order); per case the arguments and every value of the returned dict (``floater_mask_3d`` as int32).

Connectivity 18. The reference documents 18 as "face + edge adjacent", but the 3 x 3 x 3 structure it builds for it is the
6-neighbour cross, so as it stands its 18 labels exactly like its 6. This project builds what the documentation says. For
the cases with ``connectivity=18`` the generator therefore hands the reference's own ``ndimage.label`` call the face + edge
structure (``generate_binary_structure(3, 2)``) in place of that cross; everything else - thresholding, volumes,
classification, the dict - is still the reference's code. One more case, ``asis18``, records the reference untouched with
``connectivity=18``: the tests check that it equals connectivity 6.
"""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("NERF_REFERENCE_SVOX2")
if not REF:
    sys.exit("set NERF_REFERENCE_SVOX2 to the svox2 directory of the reference checkout (the one that holds opt/util)")
spec = importlib.util.spec_from_file_location("reference_advanced_metrics", os.path.join(REF, "opt", "util", "advanced_metrics.py"))
ref = importlib.util.module_from_spec(spec)
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    spec.loader.exec_module(ref)
assert ref.HAS_SCIPY, "the reference needs scipy to label"

CROSS = ref.ndimage.generate_binary_structure(3, 1)
FACES_AND_EDGES = ref.ndimage.generate_binary_structure(3, 2)
_label = ref.ndimage.label


def label_with_documented_18(input, structure=None, output=None):
    if structure is not None and np.array_equal(np.asarray(structure, dtype=bool), CROSS):
        structure = FACES_AND_EDGES
    return _label(input, structure=structure, output=output)


DEFAULTS = dict(threshold=0.01, use_density_threshold=True, min_object_size=1000, size_gap_ratio=0.2, use_adaptive=True,
                connectivity=26)


def links_of(kept, rng):
    """Kept nodes numbered in permuted order; empty nodes -1, some of them -2 and -7."""
    links = np.full(kept.shape, -1, dtype=np.int32)
    empty = np.flatnonzero(~kept.reshape(-1))
    links.reshape(-1)[empty[::5]] = -2
    links.reshape(-1)[empty[::11]] = -7
    links[kept] = rng.permutation(int(kept.sum())).astype(np.int32)
    return links


def blobs_grid(rng):
    """(56, 48, 64): three balls of about 3000 / 1400 / 1150 nodes, 1.5 % specks (some touching only by an edge or a corner),
    a shell of kept nodes around the largest ball whose density is below the threshold."""
    shape = (56, 48, 64)
    x, y, z = np.meshgrid(*(np.arange(s) for s in shape), indexing="ij")

    def ball(c, r):
        return (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2 <= r * r

    solid = ball((16, 15, 18), 9.0) | ball((38, 30, 44), 7.0) | ball((18, 34, 50), 6.5)
    shell = ball((16, 15, 18), 11.0) & ~ball((16, 15, 18), 10.0)      # kept, below the threshold, not touching the ball
    near = ball((16, 15, 18), 13.0) | ball((38, 30, 44), 9.0) | ball((18, 34, 50), 8.5)
    specks = (rng.random(shape) < 0.015) & ~near
    kept = solid | shell | specks
    links = links_of(kept, rng)
    density = np.zeros((int(kept.sum()), 1), dtype=np.float32)
    density[links[solid | specks], 0] = rng.uniform(0.02, 8.0, int((solid | specks).sum())).astype(np.float32)
    density[links[shell], 0] = rng.uniform(0.0, 0.009, int(shell.sum())).astype(np.float32)
    return links, density


def edge_grid(rng):
    """(12, 10, 14): densities exactly at float32(0.01) and float32(0.3), one ulp either side, NaN, infinities, negatives."""
    shape = (12, 10, 14)
    kept = rng.random(shape) < 0.55
    links = links_of(kept, rng)
    t1, t2 = np.float32(0.01), np.float32(0.3)
    special = np.array([t1, np.nextafter(t1, np.float32(1)), np.nextafter(t1, np.float32(0)), t2, np.nextafter(t2, np.float32(1)),
                        np.nextafter(t2, np.float32(0)), np.nan, np.inf, -np.inf, -1.0, 0.0, -0.0, 1e-30, 5.0], dtype=np.float32)
    density = special[rng.integers(0, special.size, int(kept.sum()))].reshape(-1, 1)
    return links, density


def small_grid(rng, shape, p):
    kept = rng.random(shape) < p
    links = links_of(kept, rng)
    return links, rng.uniform(0.0, 2.0, (int(kept.sum()), 1)).astype(np.float32)


def main():
    rng = np.random.default_rng(20240611)
    grids = {"blobs": blobs_grid(rng), "edge": edge_grid(rng), "dust": small_grid(rng, (9, 20, 13), 0.2),
             "empty": (np.where(np.arange(8 * 6 * 10).reshape(8, 6, 10) % 3 == 0, -3, -1).astype(np.int32),
                       np.zeros((0, 1), dtype=np.float32))}
    cases = [
        ("blobs_26", "blobs", {}),                                         # adaptive, no gap among the three balls
        ("blobs_18", "blobs", dict(connectivity=18)),
        ("blobs_6", "blobs", dict(connectivity=6)),
        ("blobs_gap", "blobs", dict(size_gap_ratio=0.5)),                    # a gap after the largest ball
        ("blobs_single", "blobs", dict(min_object_size=2000)),               # one large component only
        ("blobs_none_large", "blobs", dict(min_object_size=100000)),
        ("blobs_simple", "blobs", dict(use_adaptive=False, min_object_size=1200)),
        ("blobs_small_gap", "blobs", dict(min_object_size=3, size_gap_ratio=0.9, connectivity=6)),
        ("blobs_thresh0", "blobs", dict(threshold=0.0)),                     # no thresholding: the shell counts
        ("blobs_links_only", "blobs", dict(use_density_threshold=False, connectivity=18)),
        ("blobs_high", "blobs", dict(threshold=4.0, min_object_size=50)),
        ("edge_001", "edge", dict(threshold=0.01, min_object_size=5)),
        ("edge_03", "edge", dict(threshold=0.3, min_object_size=5, connectivity=6)),
        ("edge_neg", "edge", dict(threshold=-1.0, min_object_size=5, connectivity=18)),
        ("edge_simple", "edge", dict(threshold=0.3, min_object_size=4, use_adaptive=False, connectivity=18)),
        ("dust_26", "dust", dict(min_object_size=4)),
        ("dust_6", "dust", dict(min_object_size=2, connectivity=6, size_gap_ratio=0.6)),
        ("empty_links", "empty", {}),
        ("empty_thresh", "dust", dict(threshold=100.0)),
        ("asis18", "blobs", dict(connectivity=18)),                          # the reference untouched: labels like 6
    ]
    out = {"cases": np.array([c[0] for c in cases]), "grids": np.array([c[1] for c in cases])}
    for name, (links, density) in grids.items():
        out[f"grid_{name}_links"], out[f"grid_{name}_density"] = links, density
    for key in DEFAULTS:
        out[key] = np.array([dict(DEFAULTS, **c[2])[key] for c in cases])
    for case, name, kw in cases:
        links, density = grids[name]
        g = types.SimpleNamespace(links=torch.from_numpy(links.copy()), density_data=torch.from_numpy(density.copy()))
        ref.ndimage.label = _label if case == "asis18" else label_with_documented_18
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                res = ref.compute_FDR(g, **dict(DEFAULTS, **kw))
        finally:
            ref.ndimage.label = _label
        out[f"{case}_keys"] = np.array(list(res.keys()))
        for k, v in res.items():
            if k == "floater_mask_3d":
                assert v.max() < 2 ** 31
                v = v.astype(np.int32)
            out[f"{case}_{k}"] = np.asarray(v)
        print(f"{case}: {name} {tuple(links.shape)} {kw}: {res['num_components']} components, FDR {res['FDR']:.4f}, "
              f"{res.get('detection_method', '(empty)')}")
    path = os.path.join(HERE, "grid_components.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
