"""Writes tests/golden/grid_floater_views.npz: what the reference's ``opt/util/floater_visualization.py`` draws of one
synthetic grid from three cameras.

    NERF_REFERENCE_SVOX2=/path/to/reference/svox2 python tests/golden/make_golden_grid_floater_views.py

Runs on the CPU. The reference module is imported from the checkout, nothing of it is copied: the fixture holds arrays only.
It imports ``cv2`` at the top, which is not needed for anything but ``dilate`` and ``circle`` in the functions recorded here;
a stand-in module is installed before the import: ``dilate`` is ``scipy.ndimage.maximum_filter(mode="constant", cval=-inf)``
(OpenCV's default border for a dilation) and ``circle`` writes the colour tuple it is given into channels 0, 1, 2 of the 21
pixels ``dx^2 + dy^2 <= 5`` inside the image (the disc of include/nerf_mi355x.h, "Sparse voxel grid: floater views"). The
reference hands ``circle`` its colours in BGR order although the image is RGB; the stand-in writes what it is given, as OpenCV
does, so the recorded overlays have the reference's channel order (tests/grid_floater_views_oracle.py: ``bgr=True``).

The grid is duck-typed (``links``, ``density_data``, ``radius``, ``center``); its ``volume_render_depth_image`` returns the
depth this fixture records, the threshold depth of tests/grid_depth_oracle.py at ``sigma_thresh=0``. 24 x 20 x 28 nodes: one
blob (density 2) and nine small components around it on all sides (so that camera A sees some in front of the blob and some
behind it), three of them of density 1/16 (below ``min_density = 0.1``), the others 1/2 or 1; every density is a multiple of
1/16. Labels are ``scipy.ndimage.label``'s with 26 neighbours; afterwards six labelled nodes lose their link (-1).

Camera A: 48 x 32, fx != fy, off-centre cx / cy, a generically rotated pose outside the box; also recorded with
``render_size=(20, 30)``. Camera B stands inside the box: nodes lie behind it and fall outside the image, and some are
visible. Camera C (centred principal point, another pose outside) is the one the overlays are recorded with: the reference's
overlay functions take ``cx = width / 2`` whatever the camera says. Each pose comes from a seed that is searched until NO labelled node is ambiguous
(the oracle's conditions) under any recorded setting and no pixel of the component view sees two slots at equal depth; both
are asserted, and so is that the oracle reproduces every recorded image exactly.
"""
import contextlib
import importlib.util
import io
import os
import sys
import types

import numpy as np
import torch
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import grid_depth_oracle as DO  # noqa: E402
import grid_floater_views_oracle as FO  # noqa: E402
import grid_oracle as GO  # noqa: E402

REF = os.environ.get("NERF_REFERENCE_SVOX2")
if not REF:
    sys.exit("set NERF_REFERENCE_SVOX2 to the svox2 directory of the reference checkout (the one that holds opt/util)")


def _dilate(src, kernel, iterations=1):
    assert iterations == 1 and np.all(kernel == 1)
    return ndimage.maximum_filter(src, footprint=np.ones(kernel.shape, dtype=bool), mode="constant", cval=-np.inf)


def _circle(img, centre, radius, colour, thickness):
    assert radius == 2 and thickness == -1
    for dx, dy in FO.DISC:
        x, y = centre[0] + dx, centre[1] + dy
        if 0 <= x < img.shape[1] and 0 <= y < img.shape[0]:
            img[y, x] = colour
    return img


cv2 = types.ModuleType("cv2")
cv2.dilate, cv2.circle = _dilate, _circle
sys.modules["cv2"] = cv2
spec = importlib.util.spec_from_file_location("reference_floater_visualization",
                                              os.path.join(REF, "opt", "util", "floater_visualization.py"))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

SHAPE = (24, 20, 28)
RADIUS = np.array([1.0, 0.9, 1.1], dtype=np.float32)
CENTER = np.array([0.1, -0.05, 0.02], dtype=np.float32)
W, H = 48, 32
RENDER_SIZE = (20, 30)
MIN_VIZ_SIZE = 100      # the blob is drawn as a main object


def make_grid():
    i, j, k = np.meshgrid(*[np.arange(s) for s in SHAPE], indexing="ij")
    dens = np.zeros(SHAPE, dtype=np.float32)
    blob = ((i - 12) / 5.2) ** 2 + ((j - 10) / 4.6) ** 2 + ((k - 14) / 5.6) ** 2 <= 1.0
    dens[blob] = 2.0
    small = [((3, 10, 14), (2, 2, 1), 0.5), ((20, 9, 13), (2, 1, 2), 1.0), ((12, 2, 14), (1, 2, 2), 0.0625),
             ((11, 17, 15), (2, 1, 1), 0.5), ((12, 10, 2), (1, 1, 3), 1.0), ((13, 9, 24), (2, 2, 2), 0.0625),
             ((4, 3, 5), (1, 1, 1), 0.5), ((20, 16, 23), (2, 2, 1), 0.0625), ((5, 16, 22), (1, 2, 1), 1.0)]
    for (a, b, c), (sa, sb, sc), rho in small:
        dens[a:a + sa, b:b + sb, c:c + sc] = rho
    occupied = dens > 0
    labels, n = ndimage.label(occupied, structure=np.ones((3, 3, 3)))
    assert n == 10
    volumes = np.bincount(labels.reshape(-1))[1:]
    main_ids = np.flatnonzero(volumes >= MIN_VIZ_SIZE) + 1
    floater_ids = np.flatnonzero(volumes < MIN_VIZ_SIZE) + 1
    assert len(main_ids) == 1 and 6 <= len(floater_ids) <= 10
    # six labelled nodes lose their link: three of floaters, three of the blob's surface
    lost = [tuple(np.argwhere(labels == f)[0]) for f in floater_ids[[0, 3, 8]]] + [tuple(x) for x in np.argwhere(blob)[[0, 7, -1]]]
    kept = occupied.copy()
    for n3 in lost:
        kept[n3] = False
    rng = np.random.default_rng(5)
    links = np.full(SHAPE, -1, dtype=np.int32)
    links[kept] = rng.permutation(int(kept.sum())).astype(np.int32)
    density = np.zeros((int(kept.sum()), 1), dtype=np.float32)
    density[links[kept], 0] = dens[kept]
    assert np.array_equal(density * 16, np.round(density * 16))
    grid = {"links": links, "density_data": density, "sh_data": np.zeros((len(density), 3), dtype=np.float32),
            "radius": RADIUS, "center": CENTER}
    return grid, labels.astype(np.int32), floater_ids.astype(np.int64), main_ids.astype(np.int64)


def look_at(rng, distance, jitter):
    """A float32 [4, 4] OpenCV c2w at ``distance`` (in units of the radius) from the centre in a random direction, looking at
    a point near the centre with a random roll."""
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    pos = CENTER + distance * RADIUS * d
    target = CENTER + jitter * rng.normal(size=3)
    z = target - pos
    z /= np.linalg.norm(z)
    up = rng.normal(size=3)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, pos
    return m.astype(np.float32)


def camera_dict(c2w, fx, fy, cx, cy):
    return {"c2w": c2w, "fx": fx, "fy": fy, "cx": W * 0.5 if cx is None else cx, "cy": H * 0.5 if cy is None else cy,
            "width": W, "height": H}


def depth_of(grid, cam):
    o, d = GO.gen_rays(cam["c2w"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], W, H)
    return DO.depth(grid, o, d, threshold=0.0)[0].reshape(H, W).astype(np.float32)


SETTINGS = [(occ, rho) for occ in (True, False) for rho in (0.0, 0.1)]


def ambiguity(grid, labels, floater_ids, main_ids, cam, depth):
    """(ambiguous nodes, ties) over every labelled node and every recorded setting"""
    table, _ = FO.slot_table(labels, main_ids, floater_ids, True, 0)
    _, amb, ties = FO.component_view(grid, labels, table, cam)
    total = int(amb.sum())
    if depth is not None:
        for size in (None, RENDER_SIZE):
            for occ, rho in SETTINGS:
                total += int(FO.heatmap(grid, labels, floater_ids, cam, depth, size, occ, rho)[3].sum())
    return total, ties


def shows_what_it_should(name, grid, labels, floater_ids, cam, depth):
    """A: some floaters in front of the blob and some behind it. B: nodes behind the camera or outside the image, and still
    something visible."""
    n = FO.heatmap(grid, labels, floater_ids, cam, depth, None, True, 0.0)[2]
    if name == "A":
        return 0 < n["visible"] < n["in_view"]
    if name == "B":
        return 0 < n["visible"] and n["in_view"] < n["dense"]
    return True


def search(name, grid, labels, floater_ids, main_ids, make, first_seed):
    for seed in range(first_seed, first_seed + 200000):
        cam = make(np.random.default_rng(seed))
        if ambiguity(grid, labels, floater_ids, main_ids, cam, None) != (0, 0):
            continue
        depth = depth_of(grid, cam)
        if (ambiguity(grid, labels, floater_ids, main_ids, cam, depth) == (0, 0)
                and shows_what_it_should(name, grid, labels, floater_ids, cam, depth)):
            return seed, cam, depth
    raise AssertionError("no pose without an ambiguous node")


class RefGrid:
    def __init__(self, grid, depth):
        self.links = torch.from_numpy(grid["links"])
        self.density_data = torch.from_numpy(grid["density_data"])
        self.radius, self.center = torch.from_numpy(grid["radius"]), torch.from_numpy(grid["center"])
        self._depth = depth

    def volume_render_depth_image(self, camera, sigma_thresh=None):
        assert sigma_thresh == 0.0
        return torch.from_numpy(self._depth)


class RefCamera:
    def __init__(self, cam, cx, cy):
        self.c2w = torch.from_numpy(cam["c2w"])
        self.fx, self.fy, self.cx, self.cy = cam["fx"], cam["fy"], cx, cy
        self.width, self.height = W, H


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def main():
    grid, labels, floater_ids, main_ids = make_grid()
    fdr = {"FDR_floater_mask_3d": labels, "FDR_floater_component_ids": floater_ids, "FDR_main_component_ids": main_ids}
    out = {"links": grid["links"], "density": grid["density_data"], "radius": RADIUS, "center": CENTER, "labels": labels,
           "floater_ids": floater_ids, "main_ids": main_ids, "render_size": np.array(RENDER_SIZE),
           "min_viz_size": np.array(MIN_VIZ_SIZE)}
    specs = {
        "A": (lambda rng: camera_dict(look_at(rng, 3.2, 0.15), 40.0, 44.0, 25.3, 14.6), (25.3, 14.6)),
        "B": (lambda rng: camera_dict(look_at(rng, 0.55, 0.3), 30.0, 33.0, 22.7, 17.2), (22.7, 17.2)),
        "C": (lambda rng: camera_dict(look_at(rng, 3.0, 0.15), 42.0, 39.0, None, None), (None, None)),
    }
    left_out = 0
    for name, (make, (cx, cy)) in specs.items():
        seed, cam, depth = search(name, grid, labels, floater_ids, main_ids, make, 1000 * (ord(name) - 64))
        n_amb, ties = ambiguity(grid, labels, floater_ids, main_ids, cam, depth)
        assert n_amb == 0 and ties == 0
        left_out += n_amb + ties
        print(f"camera {name}: pose seed {seed}")
        out[f"{name}_seed"] = np.array(seed)
        out[f"{name}_c2w"] = cam["c2w"]
        out[f"{name}_intrinsics"] = np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"]], dtype=np.float64)
        out[f"{name}_centred"] = np.array(cx is None)
        out[f"{name}_depth"] = depth
        rgrid, rcam = RefGrid(grid, depth), RefCamera(cam, cx, cy)
        for size in ((None, RENDER_SIZE) if name == "A" else (None,)):
            for occ, rho in SETTINGS:
                got = quiet(ref.project_floaters_to_view, rgrid, fdr, rcam, render_size=size, filter_occluded=occ, min_density=rho)
                want, _, n, _ = FO.heatmap(grid, labels, floater_ids, cam, depth, size, occ, rho)
                assert got.dtype == np.float32 and np.array_equal(got, want), (name, size, occ, rho)
                print(f"  size {size} occluded {occ} min_density {rho}: {n}, max {got.max():.0f}")
                out[f"{name}_heat_{'size' if size else 'full'}_{int(occ)}_{int(rho > 0)}"] = got
        assert shows_what_it_should(name, grid, labels, floater_ids, cam, depth)
        if name == "A":      # some floaters are below min_density
            assert (FO.heatmap(grid, labels, floater_ids, cam, depth, None, False, 0.1)[2]["dense"]
                    < FO.heatmap(grid, labels, floater_ids, cam, depth, None, False, 0.0)[2]["dense"])
        if name == "C":
            rgb = np.random.default_rng(11).random((H, W, 3), dtype=np.float32)
            out["C_rgb"] = rgb
            multi = quiet(ref.create_multi_object_voxel_overlay, rgb, rgrid, fdr, rcam, max_points_per_object=10 ** 9, alpha=0.7,
                          show_floaters=True, min_viz_size=MIN_VIZ_SIZE)
            plain = quiet(ref.create_multi_object_voxel_overlay, rgb, rgrid, fdr, rcam, max_points_per_object=10 ** 9, alpha=0.6,
                          show_floaters=False, min_viz_size=MIN_VIZ_SIZE)
            main_only = quiet(ref.create_main_object_voxel_overlay, rgb, rgrid, fdr, rcam, max_points=10 ** 9, alpha=0.7)
            for key, got, (floaters, alpha) in (("multi", multi, (True, 0.7)), ("nofloat", plain, (False, 0.6))):
                table, n_main = FO.slot_table(labels, main_ids, floater_ids, floaters, MIN_VIZ_SIZE)
                slots, _, ties = FO.component_view(grid, labels, table, cam)
                assert ties == 0 and got.dtype == np.float32
                assert np.array_equal(got, FO.multi_object_overlay(rgb, slots, n_main, alpha, bgr=True)), key
                out[f"C_overlay_{key}"] = got
            slots, _, _ = FO.component_view(grid, labels, FO.slot_table(labels, main_ids, [], False, 0)[0], cam)
            assert np.array_equal(main_only, FO.main_object_overlay(rgb, slots, 0.7, bgr=True))
            out["C_overlay_main"] = main_only
    assert left_out == 0
    path = os.path.join(HERE, "grid_floater_views.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, 0 cases left out")


if __name__ == "__main__":
    main()
