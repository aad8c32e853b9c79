"""Floater views of the sparse voxel grid on the GPU (include/nerf_mi355x.h, "Sparse voxel grid: floater views").

Everything is compared bit for bit with tests/grid_floater_views_oracle.py, which tests/test_grid_floater_views_cpu.py holds
against the reference's recorded images; the depth map is passed in, so it is an exact input. The comparison is exact because
no candidate node is ambiguous (the oracle's conditions), which every test that compares asserts: 0 cases are left out.
Needs a real MI355X: run with ``pytest -m gpu``."""
import functools

import numpy as np
import pytest
import torch

import grid_floater_views_oracle as FO
from test_grid import cpu, gpu, make_grid
from test_grid_floater_views_cpu import (CAMERAS, HEAT_CASES, fixture_camera, fixture_grid, load_floater_fixture,
                                         oracle_component_view, oracle_heatmap, render_size)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def N():
    import nerf_projects_amd as pkg
    return pkg


def camera_of(N, cam, centred=False):
    return N.Camera(torch.from_numpy(np.asarray(cam["c2w"], dtype=np.float32)), fx=cam["fx"], fy=cam["fy"],
                    cx=None if centred else cam["cx"], cy=None if centred else cam["cy"], width=cam["width"], height=cam["height"])


def fixture_camera_gpu(N, z, name):
    return camera_of(N, fixture_camera(z, name), bool(z[f"{name}_centred"]))


def fdr_of(labels, floater_ids, main_ids, prefix=""):
    return {prefix + "floater_mask_3d": gpu(labels), prefix + "floater_component_ids": np.asarray(floater_ids),
            prefix + "main_component_ids": np.asarray(main_ids)}


@pytest.fixture(scope="module")
def fix(N):
    z = load_floater_fixture()
    return z, make_grid(N, fixture_grid(z)), fdr_of(z["labels"], z["floater_ids"], z["main_ids"])


# ---- 1. the fixture: equal to the oracle, hence to the reference ----------------------------------------------------------
@pytest.mark.parametrize("name,size,occ,rho", HEAT_CASES)
def test_heatmap_and_counters_equal_the_oracle_bit_for_bit(N, fix, name, size, occ, rho):
    z, grid, fdr = fix
    want, _, n, amb = oracle_heatmap(name, size, occ, rho)
    assert amb.sum() == 0
    cam = fixture_camera_gpu(N, z, name)
    kw = dict(render_size=render_size(z, size), filter_occluded=occ, min_density=rho, depth_map=gpu(z[f"{name}_depth"]))
    got, counts = N.project_floaters_to_view(grid, fdr, cam, return_counts=True, **kw)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == want.shape
    assert np.array_equal(cpu(got), want) and counts == n
    again = N.project_floaters_to_view(grid, fdr, cam, **kw)      # two calls: identical bits
    assert torch.equal(again, got)


@pytest.mark.parametrize("name", CAMERAS)
def test_component_view_equals_the_oracle_bit_for_bit(N, fix, name):
    z, grid, fdr = fix
    cam = fixture_camera_gpu(N, z, name)
    for floaters, viz in ((True, int(z["min_viz_size"])), (False, int(z["min_viz_size"])), (True, 0), (True, 5000)):
        want, _, amb, ties = oracle_component_view(name, floaters, viz)
        assert amb.sum() == 0 and ties == 0
        got = N.component_view(grid, fdr, cam, show_floaters=floaters, min_viz_size=viz)
        assert got.dtype == torch.int32 and tuple(got.shape) == (32, 48)
        assert np.array_equal(cpu(got), want), (floaters, viz)
        assert torch.equal(N.component_view(grid, fdr, cam, show_floaters=floaters, min_viz_size=viz), got)
    assert (want > 0).any() and set(np.unique(want)) <= {0, 1}      # min_viz_size 5000: no main object, floaters are slot 1


def test_default_depth_is_the_threshold_depth_image(N, fix):
    z, grid, fdr = fix
    for name in ("A", "B"):
        cam = fixture_camera_gpu(N, z, name)
        depth = grid.volume_render_depth_image(cam, sigma_thresh=0.0)
        want = N.project_floaters_to_view(grid, fdr, cam, min_density=0.0, depth_map=depth)
        assert torch.equal(N.project_floaters_to_view(grid, fdr, cam, min_density=0.0), want)
        assert torch.equal(N.project_floaters_to_view(grid, fdr, cam, min_density=0.0, depth_map=depth.unsqueeze(-1)), want)
    assert want.max() > 0


def test_overlays_equal_the_oracles_blend(N, fix):
    z, grid, fdr = fix
    rgb, viz = z["C_rgb"], int(z["min_viz_size"])
    for name in ("C", "A"):
        cam = fixture_camera_gpu(N, z, name)
        for floaters, alpha in ((True, 0.7), (False, 0.6)):
            slots, n_main, _, _ = oracle_component_view(name, floaters, viz)
            got = N.multi_object_overlay(gpu(rgb), grid, fdr, cam, alpha=alpha, show_floaters=floaters, min_viz_size=viz)
            assert got.dtype == torch.float32 and tuple(got.shape) == (32, 48, 3)
            assert np.array_equal(cpu(got), FO.multi_object_overlay(rgb, slots, n_main, alpha))
        slots, _, _, _ = oracle_component_view(name, False, 0)
        got = N.main_object_overlay(gpu(rgb), grid, fdr, cam, alpha=0.7)
        assert np.array_equal(cpu(got), FO.main_object_overlay(rgb, slots, 0.7))
    # the reference's image itself where nothing is painted (where something is, it differs by its channel order alone:
    # tests/test_grid_floater_views_cpu.py)
    slots, _, _, _ = oracle_component_view("C", True, viz)
    ours = cpu(N.multi_object_overlay(gpu(rgb), grid, fdr, fixture_camera_gpu(N, z, "C"), min_viz_size=viz))
    assert np.array_equal(ours[slots == 0], z["C_overlay_multi"][slots == 0])
    # the red tint: exact where nothing is divided, to one rounding of heatmap / max elsewhere
    heat = oracle_heatmap("A", False, False, 0.0)[0]
    got = cpu(N.floater_overlay_on_render(gpu(rgb), gpu(heat.copy()), alpha=0.9))
    want = FO.floater_overlay_on_render(rgb, heat, 0.9)
    assert np.array_equal(got[heat == 0], rgb[heat == 0]) and np.abs(got - want).max() <= 1e-6
    mask = heat > 0
    border = mask & ~(np.pad(mask, 1, constant_values=True)[2:, 1:-1] & np.pad(mask, 1, constant_values=True)[:-2, 1:-1]
                      & np.pad(mask, 1, constant_values=True)[1:-1, 2:] & np.pad(mask, 1, constant_values=True)[1:-1, :-2])
    assert border.any() and np.array_equal(got[border], np.broadcast_to(np.float32([1, 0, 0]), got[border].shape))
    assert torch.equal(N.floater_overlay_on_render(gpu(rgb), gpu(heat * 0)), gpu(rgb))
    assert N.floater_overlay_on_render(gpu(rgb), None) is not None


# ---- 2. end to end from compute_FDR ------------------------------------------------------------------------------------------
def test_end_to_end_from_compute_fdr_with_both_key_forms(N, fix):
    z, grid, _ = fix
    cam = fixture_camera_gpu(N, z, "A")
    depth = gpu(z["A_depth"])
    fdr = N.compute_FDR(grid, min_object_size=100)
    assert fdr["num_floaters"] >= 6 and fdr["num_main_objects"] == 1
    labels = cpu(fdr["floater_mask_3d"])
    assert ((labels > 0) <= (z["labels"] > 0)).all()      # a subset of the fixture's labelled nodes: none is ambiguous
    flat = {f"FDR_{k}": v for k, v in fdr.items()}
    for occ, rho in ((True, 0.1), (False, 0.0)):
        want, counts, n, amb = FO.heatmap(fixture_grid(z), labels, fdr["floater_component_ids"], fixture_camera(z, "A"),
                                          z["A_depth"], None, occ, rho, n_labels=fdr["num_components"])
        assert amb.sum() == 0 and n["visible"] == counts.sum() > 0
        for form in (fdr, flat):
            got, seen = N.project_floaters_to_view(grid, form, cam, filter_occluded=occ, min_density=rho, depth_map=depth,
                                                   return_counts=True)
            assert np.array_equal(cpu(got), want) and seen == n
            assert (cpu(got) > 0).sum() >= (counts > 0).sum() and cpu(got).max() == counts.max()
    table, n_main = FO.slot_table(labels, fdr["main_component_ids"], fdr["floater_component_ids"], True, 100)
    want, amb, ties = FO.component_view(fixture_grid(z), labels, table, fixture_camera(z, "A"))
    assert amb.sum() == 0 and ties == 0 and n_main == 1
    for form in (fdr, flat):
        assert np.array_equal(cpu(N.component_view(grid, form, cam, min_viz_size=100)), want)
    # min_density removes every floater: a zero heatmap, nothing counted
    got, seen = N.project_floaters_to_view(grid, fdr, cam, min_density=100.0, depth_map=depth, return_counts=True)
    assert tuple(got.shape) == (32, 48) and not cpu(got).any() and seen == {"in_view": 0, "dense": 0, "visible": 0}
    # no floater id, no label tensor: None
    none = N.compute_FDR(grid, min_object_size=1, use_adaptive=False)
    assert none["num_floaters"] == 0 and N.project_floaters_to_view(grid, none, cam) is None
    assert N.project_floaters_to_view(grid, {"FDR": 0.0}, cam) is None and N.component_view(grid, {"FDR": 0.0}, cam) is None
    rgb = gpu(z["C_rgb"])
    assert N.multi_object_overlay(rgb, grid, {"FDR": 0.0}, cam) is rgb and N.main_object_overlay(rgb, grid, {}, cam) is rgb


# ---- 3. a larger volume: the early-out, many blocks, contended pixels, the palette's wrap-around ---------------------------------
BIG_SEED = 25     # the camera pose; chosen so that the oracle reports no ambiguous node (asserted below)


@functools.lru_cache(maxsize=None)
def big_case(seed):
    """64^3 nodes (1024 blocks of 256), 3000 labels scattered over a tenth of them, of which 60 are floaters and 16 main
    components (14 of them reach min_viz_size = 8: more than the palette's 12); a 96 x 64 camera outside the box and an
    arbitrary depth map. Everything but the pose comes from fixed seeds."""
    rng = np.random.default_rng(7)
    shape = (64, 64, 64)
    labels = np.where(rng.random(shape) < 0.1, rng.integers(1, 3001, shape), 0).astype(np.int32)
    kept = rng.random(shape) < 0.8
    links = np.full(shape, -1, dtype=np.int32)
    links[kept] = rng.permutation(int(kept.sum())).astype(np.int32)
    density = (rng.integers(0, 48, (int(kept.sum()), 1)) / 16).astype(np.float32)
    grid = {"links": links, "density_data": density, "sh_data": np.zeros((len(density), 3), dtype=np.float32),
            "radius": np.array([1.0, 1.1, 0.9], dtype=np.float32), "center": np.array([0.05, 0.0, -0.1], dtype=np.float32)}
    volumes = np.bincount(labels.reshape(-1), minlength=3001)
    ids = rng.permutation(3000) + 1
    floater_ids = np.sort(ids[:60])
    big = ids[60:][volumes[ids[60:]] >= 8][:14]
    small = ids[60:][volumes[ids[60:]] < 8][:2]
    main_ids = np.concatenate([big[:7], small, big[7:]])
    assert len(big) == 14 and len(small) == 2
    depth = rng.uniform(2.0, 4.0, (64, 96)).astype(np.float32)
    depth[rng.random((64, 96)) < 0.1] = 0.0
    prng = np.random.default_rng(seed)
    d = prng.normal(size=3)
    d /= np.linalg.norm(d)
    pos = grid["center"] + 3.0 * d
    zax = (grid["center"] + 0.1 * prng.normal(size=3)) - pos
    zax /= np.linalg.norm(zax)
    xax = np.cross(prng.normal(size=3), zax)
    xax /= np.linalg.norm(xax)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = xax, np.cross(zax, xax), zax, pos
    cam = {"c2w": c2w.astype(np.float32), "fx": 95.0, "fy": 90.0, "cx": 47.3, "cy": 33.4, "width": 96, "height": 64}
    return grid, labels, floater_ids, main_ids, cam, depth


def big_ambiguity(seed):
    """ambiguous nodes + ties of everything test_a_larger_volume compares"""
    grid, labels, floater_ids, main_ids, cam, depth = big_case(seed)
    total = sum(int(FO.heatmap(grid, labels, floater_ids, cam, depth, None, occ, rho)[3].sum()) for occ in (True, False)
                for rho in (0.0, 0.9))
    table, _ = FO.slot_table(labels, main_ids, floater_ids, True, 8)
    _, amb, ties = FO.component_view(grid, labels, table, cam)
    return total + int(amb.sum()) + ties


def test_a_larger_volume_against_the_oracle_exactly(N):
    assert big_ambiguity(BIG_SEED) == 0      # 0 cases left out
    g, labels, floater_ids, main_ids, cam, depth = big_case(BIG_SEED)
    grid = make_grid(N, g)
    fdr = fdr_of(labels, floater_ids, main_ids, "FDR_")
    camera = camera_of(N, cam)
    for occ in (True, False):
        for rho in (0.0, 0.9):
            want, counts, n, _ = FO.heatmap(g, labels, floater_ids, cam, depth, None, occ, rho)
            got, seen = N.project_floaters_to_view(grid, fdr, camera, filter_occluded=occ, min_density=rho, depth_map=gpu(depth),
                                                   return_counts=True)
            assert np.array_equal(cpu(got), want) and seen == n
    assert counts.max() >= 2 and 0 < n["dense"] < (np.isin(labels, floater_ids)).sum()      # contended pixels; a real filter
    table, n_main = FO.slot_table(labels, main_ids, floater_ids, True, 8)
    want, _, _ = FO.component_view(g, labels, table, cam)
    assert n_main == 14 and {13, 14, 15} <= set(np.unique(want))
    got = N.component_view(grid, fdr, camera, min_viz_size=8)
    assert np.array_equal(cpu(got), want)
    assert torch.equal(N.component_view(grid, fdr, camera, min_viz_size=8), got)
    rgb = np.random.default_rng(3).random((64, 96, 3), dtype=np.float32)
    over = cpu(N.multi_object_overlay(gpu(rgb), grid, fdr, camera, alpha=0.7, min_viz_size=8))
    assert np.array_equal(over, FO.multi_object_overlay(rgb, want, n_main, 0.7))
    # slot 13 wraps to the palette's first colour, slot 15 is the floaters' red
    first = FO.blend(rgb, np.broadcast_to(FO.OBJECT_COLORS[0], rgb.shape), want == 13, 0.7)
    red = FO.blend(rgb, np.broadcast_to(FO.FLOATER_COLOR, rgb.shape), want == 15, 0.7)
    assert np.array_equal(over[want == 13], first[want == 13]) and np.array_equal(over[want == 15], red[want == 15])


# ---- 4. argument errors --------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_grid_usable(N, fix):
    z, grid, fdr = fix
    cam = fixture_camera_gpu(N, z, "A")
    depth = gpu(z["A_depth"])
    before = N.project_floaters_to_view(grid, fdr, cam, depth_map=depth)
    on_cpu = dict(fdr, floater_mask_3d=torch.from_numpy(z["labels"]))
    other = dict(fdr, floater_mask_3d=gpu(z["labels"][:, :, :-1]))
    wrong_type = dict(fdr, floater_mask_3d=gpu(z["labels"].astype(np.int64)))
    ndc = fixture_camera_gpu(N, z, "A")
    ndc.ndc_coeffs = (1.0, 1.0)
    for fn in (lambda f, c: N.project_floaters_to_view(grid, f, c, depth_map=depth), lambda f, c: N.component_view(grid, f, c),
               lambda f, c: N.multi_object_overlay(gpu(z["C_rgb"]), grid, f, c)):
        with pytest.raises(RuntimeError, match="CPU"):
            fn(on_cpu, cam)
        with pytest.raises(ValueError, match="links"):
            fn(other, cam)
        with pytest.raises(TypeError, match="int32"):
            fn(wrong_type, cam)
        with pytest.raises(NotImplementedError, match="NDC"):
            fn(fdr, ndc)
    with pytest.raises(RuntimeError, match="CPU"):
        N.project_floaters_to_view(grid, fdr, cam, depth_map=torch.from_numpy(z["A_depth"]))
    with pytest.raises(ValueError, match="depth_map"):
        N.project_floaters_to_view(grid, fdr, cam, depth_map=depth[:, :-1])
    with pytest.raises(RuntimeError, match="heatmap 0 x 4"):
        N.project_floaters_to_view(grid, fdr, cam, render_size=(4, 0), depth_map=depth)
    with pytest.raises(ValueError, match="start at 1"):
        N.project_floaters_to_view(grid, dict(fdr, floater_component_ids=[0, 2]), cam, depth_map=depth)
    with pytest.raises(RuntimeError, match="CPU"):
        N.multi_object_overlay(torch.from_numpy(z["C_rgb"]), grid, fdr, cam)
    with pytest.raises(TypeError, match="SparseGrid"):
        N.component_view(None, fdr, cam)
    assert torch.equal(N.project_floaters_to_view(grid, fdr, cam, depth_map=depth), before)
    assert torch.isfinite(grid.volume_render_image(cam)).all()
