"""Floater views of the sparse voxel grid, the parts that need no GPU: the numpy restatement (tests/grid_floater_views_oracle.py)
against what the reference's floater_visualization.py recorded (tests/golden/grid_floater_views.npz, written by
tests/golden/make_golden_grid_floater_views.py), the fixture's ambiguity count, the C ABI of the two entry points and the
generated code of csrc/grid_floater_kernels.hip."""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_floater_views_oracle as FO  # noqa: E402
from grid_testlib import assert_structs_match_c_header, compile_kernels_to_asm  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "grid_floater_views.npz")
CAMERAS = ("A", "B", "C")
SETTINGS = [(occ, rho) for occ in (True, False) for rho in (0.0, 0.1)]
HEAT_CASES = [(name, size, occ, rho) for name in CAMERAS for size in ((False, True) if name == "A" else (False,))
              for occ, rho in SETTINGS]
NEW_STRUCTS = {"nerf_grid_floater_heatmap_args": "GridFloaterHeatmapArgs", "nerf_grid_component_view_args": "GridComponentViewArgs"}
NEW_SYMBOLS = ("nerf_grid_floater_heatmap", "nerf_grid_component_view")


@functools.lru_cache(maxsize=None)
def load_floater_fixture():
    return dict(np.load(FIXTURE))      # (allow_pickle is off: arrays only)


def fixture_grid(z):
    return {"links": z["links"], "density_data": z["density"], "sh_data": np.zeros((len(z["density"]), 3), dtype=np.float32),
            "radius": z["radius"], "center": z["center"]}


def fixture_camera(z, name):
    fx, fy, cx, cy = z[f"{name}_intrinsics"].tolist()
    return {"c2w": z[f"{name}_c2w"], "fx": fx, "fy": fy, "cx": cx, "cy": cy, "width": 48, "height": 32}


def render_size(z, size):
    return tuple(int(v) for v in z["render_size"]) if size else None


def heat_key(name, size, occ, rho):
    return f"{name}_heat_{'size' if size else 'full'}_{int(occ)}_{int(rho > 0)}"


@functools.lru_cache(maxsize=None)
def oracle_heatmap(name, size, occ, rho):
    """(heatmap, counts, counters, ambiguous) of the restatement on the fixture; computed once, shared with the GPU tests"""
    z = load_floater_fixture()
    out = FO.heatmap(fixture_grid(z), z["labels"], z["floater_ids"], fixture_camera(z, name), z[f"{name}_depth"],
                     render_size(z, size), occ, rho)
    for a in (out[0], out[1], out[3]):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_component_view(name, show_floaters, min_viz_size):
    """(slots, n_main_drawn, ambiguous, ties)"""
    z = load_floater_fixture()
    table, n_main = FO.slot_table(z["labels"], z["main_ids"], z["floater_ids"], show_floaters, min_viz_size)
    slots, amb, ties = FO.component_view(fixture_grid(z), z["labels"], table, fixture_camera(z, name))
    slots.setflags(write=False)
    return slots, n_main, amb, ties


def test_fixture_holds_arrays_only_and_is_small():
    assert os.path.getsize(FIXTURE) < 1 << 20
    z = load_floater_fixture()
    assert z["links"].shape == (24, 20, 28) == z["labels"].shape and z["labels"].dtype == np.int32
    assert 6 <= len(z["floater_ids"]) <= 10 and len(z["main_ids"]) == 1
    labelled = z["labels"] > 0
    assert ((z["links"] < 0) & labelled).sum() == 6                       # labelled nodes without a link
    assert np.array_equal(z["density"] * 16, np.round(z["density"] * 16))
    rho = np.where(z["links"] >= 0, z["density"][np.maximum(z["links"], 0), 0], 0)
    floater = np.isin(z["labels"], z["floater_ids"])
    assert (rho[floater] < 0.1).any() and (rho[floater] >= 0.1).any()
    assert not bool(z["A_centred"]) and not bool(z["B_centred"]) and bool(z["C_centred"])
    fx, fy, cx, cy = z["A_intrinsics"]
    assert fx != fy and cx != 24.0 and cy != 16.0


@pytest.mark.parametrize("name,size,occ,rho", HEAT_CASES)
def test_oracle_reproduces_the_references_heatmaps_exactly(name, size, occ, rho):
    z = load_floater_fixture()
    want = z[heat_key(name, size, occ, rho)]
    got, counts, n, _ = oracle_heatmap(name, size, occ, rho)
    assert got.dtype == np.float32 and got.shape == want.shape == (render_size(z, size) or (32, 48))
    assert np.array_equal(got, want)
    assert n["visible"] == counts.sum() and n["visible"] <= n["in_view"] <= n["dense"]
    if not occ:
        assert n["visible"] == n["in_view"]


def test_fixture_cameras_show_what_they_are_there_for():
    a = oracle_heatmap("A", False, True, 0.0)[2]
    assert 0 < a["visible"] < a["in_view"]                                # floaters in front of the blob and behind it
    assert oracle_heatmap("A", False, False, 0.1)[2]["dense"] < a["dense"]      # floaters below min_density
    b = oracle_heatmap("B", False, True, 0.0)[2]
    assert 0 < b["visible"] and b["in_view"] < b["dense"]                # nodes behind the camera or outside the image
    s = oracle_heatmap("A", True, False, 0.0)[2]
    assert 0 < s["in_view"] < oracle_heatmap("A", False, False, 0.0)[2]["in_view"]      # render_size cuts some off


def test_oracle_overlays_equal_the_references_exactly():
    """The reference hands OpenCV BGR tuples for an RGB image: ``bgr=True`` is its channel order, the geometry, the depth test
    and the blend are compared exactly."""
    z = load_floater_fixture()
    rgb, viz = z["C_rgb"], int(z["min_viz_size"])
    for key, floaters, alpha in (("multi", True, 0.7), ("nofloat", False, 0.6)):
        slots, n_main, _, ties = oracle_component_view("C", floaters, viz)
        assert ties == 0 and n_main == 1
        assert set(np.unique(slots)) == ({0, 1, 2} if floaters else {0, 1})
        got = FO.multi_object_overlay(rgb, slots, n_main, alpha, bgr=True)
        assert got.dtype == np.float32 and np.array_equal(got, z[f"C_overlay_{key}"]), key
    slots, _, _, _ = oracle_component_view("C", False, 0)
    assert np.array_equal(FO.main_object_overlay(rgb, slots, 0.7, bgr=True), z["C_overlay_main"])


def test_fixture_has_no_ambiguous_node_and_no_tie():
    """0 cases left out: no labelled node of the fixture is ambiguous from any camera under any recorded setting."""
    total = 0
    for name in CAMERAS:
        _, _, amb, ties = oracle_component_view(name, True, 0)      # every labelled node is a candidate here
        assert len(amb) == (load_floater_fixture()["labels"] > 0).sum()
        total += int(amb.sum()) + ties
    for case in HEAT_CASES:
        total += int(oracle_heatmap(*case)[3].sum())
    assert total == 0


def test_oracle_flags_ambiguous_nodes():
    """The conditions themselves: a node on a pixel boundary, at the camera plane, at the occlusion bound and at min_density."""
    grid = {"links": np.zeros((2, 2, 2), dtype=np.int32), "density_data": np.array([[0.1]], dtype=np.float32),
            "radius": np.ones(3, dtype=np.float32), "center": np.zeros(3, dtype=np.float32)}
    labels = np.zeros((2, 2, 2), dtype=np.int32)
    labels[1, 1, 1] = 1      # p = (0, 0, 0)
    cam = {"c2w": np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -2.0]]), "fx": 10.0, "fy": 10.0, "cx": 4.0, "cy": 4.5,
           "width": 8, "height": 8}
    depth = np.full((8, 8), 1.95, dtype=np.float32)
    assert FO.heatmap(grid, labels, [1], cam, depth, None, False, 0.0)[3].tolist() == [True]      # x = 4.0
    cam["cx"] = 4.5
    assert FO.heatmap(grid, labels, [1], cam, depth, None, False, 0.0)[3].tolist() == [False]
    assert FO.heatmap(grid, labels, [1], cam, depth, None, True, 0.0)[3].tolist() == [True]       # q2 = 2 = d + 0.05
    assert FO.heatmap(grid, labels, [1], cam, depth * 0 + 1.0, None, True, 0.0)[3].tolist() == [False]
    assert FO.heatmap(grid, labels, [1], cam, depth, None, False, 0.1)[3].tolist() == [True]      # rho = min_density
    cam["c2w"][2, 3] = 0.0005
    assert FO.heatmap(grid, labels, [1], cam, depth, None, False, 0.0)[3].tolist() == [True]      # q2 near 0


def test_floater_structs_match_a_c_compile_of_the_header(tmp_path):
    from nerf_projects_amd import _lib
    consts = assert_structs_match_c_header(tmp_path, NEW_STRUCTS, extra_prints=[
        'printf("consts slots %d\\n", NERF_GRID_FLOATER_COUNTER_INTS);'])
    assert consts == {"consts": {"slots": _lib.NERF_GRID_FLOATER_COUNTER_INTS}}


def test_floater_calls_refuse_bad_arguments_before_any_device_call():
    """Every refusal here comes before a handle is dereferenced: the grid pointer is a fake."""
    import nerf_projects_amd  # noqa: F401
    from nerf_projects_amd import _lib
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in _lib.EXPORTS
    fake = C.c_void_p(0x1000)
    err = lambda: lib.nerf_last_error().decode()      # noqa: E731

    def camera():
        c = _lib.GridCamera()
        c.c2w[:] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
        c.fx = c.fy = 10.0
        c.cx = c.cy = 4.0
        c.width = c.height = 8
        return c

    def fill(a):
        a.labels, a.table, a.n_labels = 0x2000, 0x3000, 3
        a.radius[:], a.center[:] = [1, 1, 1], [0, 0, 0]
        a.w2c[:] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
        return a

    for fn, cls in ((lib.nerf_grid_floater_heatmap, _lib.GridFloaterHeatmapArgs), (lib.nerf_grid_component_view, _lib.GridComponentViewArgs)):
        cam, a = camera(), fill(cls())
        assert fn(None, C.byref(cam), C.byref(a)) == -1 and "NULL grid" in err()
        assert fn(fake, C.byref(cam), None) == -1 and "NULL" in err()
        assert fn(fake, None, C.byref(a)) == -1 and "nerf_grid_camera is NULL" in err()
        a.struct_size -= 8
        assert fn(fake, C.byref(cam), C.byref(a)) == -1 and "struct_size" in err()
        a = fill(cls())
        cam.struct_size += 4
        assert fn(fake, C.byref(cam), C.byref(a)) == -1 and "nerf_grid_camera.struct_size" in err()
        cam = camera()
        cam.width = 0
        assert fn(fake, C.byref(cam), C.byref(a)) == -1 and "camera" in err()
        cam = camera()
        a.labels = None
        assert fn(fake, C.byref(cam), C.byref(a)) == -1 and "labels and table are required" in err()
        a = fill(cls())
        a.n_labels = -1
        assert fn(fake, C.byref(cam), C.byref(a)) == -1 and "n_labels" in err()
        a = fill(cls())
        a.radius[1] = 0.0
        assert fn(fake, C.byref(cam), C.byref(a)) == -1 and "radius" in err()
        a = fill(cls())
        a.w2c[5] = float("nan")
        assert fn(fake, C.byref(cam), C.byref(a)) == -1 and "w2c[5]" in err()
        a = fill(cls())      # and no outputs
        if cls is _lib.GridFloaterHeatmapArgs:
            a.out_width, a.out_height = 8, 0
            assert fn(fake, C.byref(cam), C.byref(a)) == -1 and "heatmap 8 x 0" in err()
            a.out_height = 8
            a.filter_occluded = 1
            assert fn(fake, C.byref(cam), C.byref(a)) == -1 and "needs depth" in err()
            a.filter_occluded = 0
            a.min_density = float("nan")
            assert fn(fake, C.byref(cam), C.byref(a)) == -1 and "min_density" in err()
            a.min_density = 0.1
            assert fn(fake, C.byref(cam), C.byref(a)) == -1 and "counts, counters, counter_slots and heatmap are required" in err()
        else:
            assert fn(fake, C.byref(cam), C.byref(a)) == -1 and "keys and slots are required" in err()


def test_floater_kernels_use_integer_atomics_only_no_scratch_and_no_inline_assembly(tmp_path):
    text, asm, build = compile_kernels_to_asm(tmp_path, "grid_floater_kernels.hip")
    assert "grid_floater_kernels.hip" in build.SOURCES and "grid_floater_api.cpp" in build.SOURCES
    assert any(h.endswith("grid_floater_internal.h") for h in build.HEADERS)
    assert not re.search(r"\basm\b|__asm", text)
    kernels = re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M)
    assert len(kernels) == 4, kernels
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)
    assert len(sizes) == len(kernels) and all(int(s) == 0 for s in sizes), sizes
    lds = re.findall(r"\.group_segment_fixed_size:\s*(\d+)", asm)
    assert all(int(s) == 0 for s in lds), lds
    assert "cmpswap" not in asm and not re.search(r"atomic\w*_f(32|64)", asm)      # no CAS loop, no float atomic
    assert re.search(r"\bglobal_atomic_add\b", asm) and re.search(r"\bglobal_atomic_umin_x2\b", asm)
    vgprs = [int(v) for v in re.findall(r"\.vgpr_count:\s*(\d+)", asm)]
    print("vgprs per kernel:", dict(zip(kernels, vgprs)))
    assert max(vgprs) <= 64      # 8 waves per SIMD
