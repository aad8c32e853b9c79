"""Connected components and floater detection on a sparse voxel grid, the parts that need no GPU: the numpy restatement
(tests/grid_components_oracle.py) against the reference's recorded ``compute_FDR`` (tests/golden/grid_components.npz) and
against a flood fill, the host half of the product (classification of the volumes, the metric dicts), the C ABI of the new
entry points, and the generated code of csrc/grid_components_kernels.hip."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_components_oracle as CO  # noqa: E402
from grid_testlib import assert_structs_match_c_header, compile_kernels_to_asm  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "grid_components.npz")
CASES = ("blobs_26", "blobs_18", "blobs_6", "blobs_gap", "blobs_single", "blobs_none_large", "blobs_simple", "blobs_small_gap",
         "blobs_thresh0", "blobs_links_only", "blobs_high", "edge_001", "edge_03", "edge_neg", "edge_simple", "dust_26", "dust_6",
         "empty_links", "empty_thresh")


def case_inputs(z, case):
    _, grid, kw = next(c for c in CO.fixture_cases(z) if c[0] == case)
    return z[f"grid_{grid}_links"], z[f"grid_{grid}_density"], kw


def test_fixture_holds_arrays_only_is_small_and_covers_the_cases():
    assert os.path.getsize(GOLDEN) < 1 << 20
    z = np.load(GOLDEN)      # (allow_pickle is off: arrays only)
    assert tuple(c[0] for c in CO.fixture_cases(z)) == CASES + ("asis18",)
    links = z["grid_blobs_links"]
    assert len(set(links.shape)) == 3 and all(48 <= s <= 64 for s in links.shape)      # not cubic
    assert (links < -1).any() and (z["grid_edge_links"] < -1).any()
    res = {c: CO.fixture_result(z, c) for c in CASES}
    counts = [res[c]["num_components"] for c in ("blobs_6", "blobs_18", "blobs_26")]
    assert counts[0] > counts[1] > counts[2] > 100, counts      # the three connectivities differ on the same volume
    vol = np.bincount(res["blobs_26"]["floater_mask_3d"].reshape(-1))[1:]
    assert 2 <= (vol > 1000).sum() <= 3 and (vol < 10).sum() > 1000      # blobs and many specks
    methods = " | ".join(res[c]["detection_method"] for c in CASES if "detection_method" in res[c])
    for word in ("adaptive_gap", "adaptive_nogap", "adaptive_single (1 main", "adaptive_single (0 main", "simple_threshold"):
        assert word in methods, word
    for c in ("empty_links", "empty_thresh"):
        assert tuple(res[c].keys()) == CO.EMPTY_KEYS and res[c]["sparsity"] == 1.0
    # the edge grid holds float32(threshold) itself, its two neighbours, and values that are not finite
    d = z["grid_edge_density"][:, 0]
    for t in (np.float32(0.01), np.float32(0.3)):
        for v in (t, np.nextafter(t, np.float32(1)), np.nextafter(t, np.float32(0))):
            assert (d == v).any()
    assert np.isnan(d).any() and np.isinf(d).any()
    kws = [case_inputs(z, c)[2] for c in CASES]
    assert any(k["threshold"] == 0 for k in kws) and any(not k["use_density_threshold"] for k in kws)
    assert any(not k["use_adaptive"] for k in kws)


@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_the_reference(case):
    z = np.load(GOLDEN)
    links, density, kw = case_inputs(z, case)
    got = CO.compute_fdr(links, density, **kw)
    want = CO.fixture_result(z, case)
    CO.assert_same_result(got, want, case)
    if got["num_components"]:
        vol = CO.volumes(got["floater_mask_3d"], got["num_components"])
        assert vol.dtype == np.int64 and vol.sum() == want["total_volume"] and vol.min() >= 1
        occ = CO.occupancy(links, density, kw["threshold"], kw["use_density_threshold"])
        assert np.array_equal(got["floater_mask_3d"] > 0, occ)


def test_the_reference_as_it_stands_labels_18_like_6():
    """The reference builds the 6-neighbour cross for connectivity 18 (its documentation says faces + edges, which is what
    this project and the 18-cases of the fixture do): recorded untouched, its 18 is the restatement's 6."""
    z = np.load(GOLDEN)
    links, density, kw = case_inputs(z, "asis18")
    assert kw["connectivity"] == 18
    got = CO.compute_fdr(links, density, **dict(kw, connectivity=6))
    got["connectivity"] = 18
    CO.assert_same_result(got, CO.fixture_result(z, "asis18"), "asis18")
    assert CO.fixture_result(z, "asis18")["num_components"] != CO.fixture_result(z, "blobs_18")["num_components"]


def flood_fill(occ, connectivity):
    """Labels by a depth-first fill from every unlabelled node in C order: the numbering by first occurrence."""
    most = {6: 1, 18: 2, 26: 3}[connectivity]
    offs = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)
            if (a, b, c) != (0, 0, 0) and abs(a) + abs(b) + abs(c) <= most]
    labels = np.zeros(occ.shape, dtype=np.int32)
    n = 0
    for start in zip(*np.nonzero(occ)):
        if labels[start]:
            continue
        n += 1
        labels[start] = n
        stack = [start]
        while stack:
            x, y, z = stack.pop()
            for a, b, c in offs:
                q = (x + a, y + b, z + c)
                if all(0 <= q[i] < occ.shape[i] for i in range(3)) and occ[q] and not labels[q]:
                    labels[q] = n
                    stack.append(q)
    return labels, n


def test_restated_labelling_is_a_flood_fill_in_c_order():
    rng = np.random.default_rng(3)
    for shape, p in (((7, 9, 11), 0.3), ((6, 5, 8), 0.6), ((2, 2, 40), 0.5), ((10, 3, 4), 0.15), ((4, 4, 4), 1.0), ((3, 3, 3), 0.0)):
        occ = rng.random(shape) < p
        counts = []
        for conn in (6, 18, 26):
            labels, n = CO.label(occ, conn)
            want, m = flood_fill(occ, conn)
            assert n == m and np.array_equal(labels, want), (shape, conn)
            first = [np.flatnonzero(labels.reshape(-1) == k)[0] for k in range(1, n + 1)]
            assert first == sorted(first)
            counts.append(n)
        assert counts[0] >= counts[1] >= counts[2]
    # no wrap-around: two opposite faces are two components; a checkerboard is dust for 6 and one piece for 18 and 26
    occ = np.zeros((4, 5, 6), dtype=bool)
    occ[0] = occ[-1] = True
    assert CO.label(occ, 26)[1] == 2
    i, j, k = np.indices((6, 6, 6))
    board = (i + j + k) % 2 == 0
    assert CO.label(board, 6)[1] == board.sum() and CO.label(board, 18)[1] == 1 and CO.label(board, 26)[1] == 1
    with pytest.raises(ValueError):
        CO.label(board, 8)


@pytest.mark.parametrize("case", [c for c in CASES if not c.startswith("empty")])
def test_product_classification_of_the_recorded_volumes(case):
    """The host half of compute_FDR: from the reference's component volumes to its dict, every value with ==."""
    from nerf_projects_amd import grid_components as GC
    z = np.load(GOLDEN)
    links, _, kw = case_inputs(z, case)
    want = CO.fixture_result(z, case)
    vol = np.bincount(want["floater_mask_3d"].reshape(-1))[1:].astype(np.int64)
    got = GC.fdr_from_volumes(vol, list(links.shape), kw["connectivity"], kw["min_object_size"], kw["size_gap_ratio"],
                              kw["use_adaptive"])
    got["floater_mask_3d"] = want["floater_mask_3d"]
    assert set(got) == set(want)
    CO.assert_same_result({k: got[k] for k in want}, want, case)
    # ties: any order of equal volumes gives the same classification
    perm = np.random.default_rng(1).permutation(vol.size)
    fl, n_main, method = GC.classify_components(vol[perm], kw["min_object_size"], kw["size_gap_ratio"], kw["use_adaptive"])
    fl0, n_main0, method0 = GC.classify_components(vol, kw["min_object_size"], kw["size_gap_ratio"], kw["use_adaptive"])
    assert np.array_equal(fl, fl0[perm]) and n_main == n_main0 and method == method0


def test_empty_volumes_give_the_short_dict_and_the_metric_dicts_have_the_reference_keys():
    import nerf_projects_amd as N
    from nerf_projects_amd import grid_components as GC
    out = GC.fdr_from_volumes(np.zeros(0, np.int64), [4, 4, 4], 26)
    assert tuple(out.keys()) == CO.EMPTY_KEYS and out["FDR"] == 0.0 and out["sparsity"] == 1.0
    m = N.compute_MCQ(psnr=28.5, peak_gpu_memory_mb=2048.0)
    assert list(m) == ["MCQ", "peak_gpu_gb", "peak_gpu_mb", "psnr", "memory_per_db"]
    assert m["MCQ"] == 2.0 / 28.5 == m["memory_per_db"] and m["peak_gpu_gb"] == 2.0 and m["peak_gpu_mb"] == 2048.0
    assert N.compute_MCQ(0.0, 100.0)["MCQ"] == 0.0
    a = N.compute_all_advanced_metrics(None, 30.0, compute_fdr=False, peak_gpu_memory_mb=3072.0, verbose=False)
    assert a == {"MCQ_MCQ": 0.1, "MCQ_peak_gpu_gb": 3.0, "MCQ_peak_gpu_mb": 3072.0, "MCQ_psnr": 30.0, "MCQ_memory_per_db": 0.1,
                 "MCQ": 0.1}
    assert N.compute_all_advanced_metrics(None, 30.0, compute_fdr=False, verbose=False) == {}


def test_refusals_without_a_gpu():
    import nerf_projects_amd as N
    from nerf_projects_amd import grid_components as GC
    with pytest.raises(TypeError):
        N.compute_FDR(object())
    with pytest.raises(TypeError):
        N.remove_floaters("grid")
    with pytest.raises(TypeError):
        N.label_components(None, connectivity=6)
    for bad in (8, 0, 27, True, "26"):
        with pytest.raises(ValueError, match="connectivity"):
            N.label_components(object(), connectivity=bad)      # refused before the grid is looked at
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GC.label_mask(torch.zeros((4, 4, 4), dtype=torch.bool))
    assert hasattr(N.GridTrainer, "remove_floaters")


def test_product_imports_neither_scipy_nor_the_oracle():
    pkg = os.path.join(ROOT, "nerf-projects_amd")
    for name in os.listdir(pkg):
        if name.endswith(".py"):
            text = open(os.path.join(pkg, name)).read()
            assert not re.search(r"^\s*(import|from)\s+scipy", text, re.M), name
            assert "grid_components_oracle" not in text, name
    code = ("import sys; sys.path.insert(0, %r); import nerf_projects_amd; from nerf_projects_amd import grid_components; "
            "bad = [m for m in sys.modules if m.split('.')[0] in ('scipy', 'oracle', 'grid_components_oracle')]; "
            "assert not bad, bad" % ROOT)
    subprocess.run([sys.executable, "-c", code], check=True)


# ---- C ABI ------------------------------------------------------------------------------------------------------------
NEW_STRUCTS = {"nerf_grid_occupancy_args": "GridOccupancyArgs", "nerf_grid_label_args": "GridLabelArgs",
               "nerf_grid_copy_rows_args": "GridCopyRowsArgs"}
NEW_SYMBOLS = ("nerf_grid_components_occupancy", "nerf_grid_components_workspace", "nerf_grid_components_label",
               "nerf_grid_components_finish", "nerf_grid_components_volumes", "nerf_grid_components_keep", "nerf_grid_copy_rows")


def test_component_structs_match_a_c_compile_of_the_header(tmp_path):
    import nerf_projects_amd  # noqa: F401
    from nerf_projects_amd import _lib
    code = assert_structs_match_c_header(tmp_path, NEW_STRUCTS, extra_prints=['printf("code internal %d\\n", NERF_E_INTERNAL);'])
    assert code == {"code": {"internal": _lib.NERF_E_INTERNAL}} and _lib.NERF_E_INTERNAL == -5


def test_component_calls_refuse_bad_arguments_before_any_device_call():
    """Every refusal here comes before a handle is dereferenced or a kernel launched: the pointers are fakes."""
    import nerf_projects_amd  # noqa: F401
    from nerf_projects_amd import _lib
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in _lib.EXPORTS
    fake = C.c_void_p(0x1000)
    err = lambda: lib.nerf_last_error().decode()      # noqa: E731

    o = _lib.GridOccupancyArgs()
    assert lib.nerf_grid_components_occupancy(None, C.byref(o)) == -1 and "NULL grid" in err()
    assert lib.nerf_grid_components_occupancy(fake, None) == -1 and "NULL" in err()
    assert lib.nerf_grid_components_occupancy(fake, C.byref(o)) == -1 and "required" in err()
    o.threshold = float("nan")
    assert lib.nerf_grid_components_occupancy(fake, C.byref(o)) == -1 and "NaN" in err()
    o.struct_size = 3
    assert lib.nerf_grid_components_occupancy(fake, C.byref(o)) == -1 and "struct_size" in err()

    assert lib.nerf_grid_components_workspace(0) == 0 and lib.nerf_grid_components_workspace(1024) == 1
    assert lib.nerf_grid_components_workspace(1025) == 2 and lib.nerf_grid_components_workspace(1 << 30) == 1 << 20
    a = _lib.GridLabelArgs()
    a.reso[:] = [4, 4, 4]
    a.connectivity = 26
    assert lib.nerf_grid_components_label(None, C.byref(a)) == -1 and "NULL context" in err()
    assert lib.nerf_grid_components_label(fake, None) == -1 and "NULL" in err()
    assert lib.nerf_grid_components_label(fake, C.byref(a)) == -1 and "required" in err()
    a.occupied = a.parent = a.block_offsets = a.labels = a.status = 0x1000
    assert lib.nerf_grid_components_label(fake, C.byref(a)) == -1 and "different buffers" in err()
    for bad in (0, 8, 27, -6):
        a.connectivity = bad
        assert lib.nerf_grid_components_label(fake, C.byref(a)) == -1 and "connectivity" in err()
    a.connectivity = 6
    a.reso[:] = [4, 1, 4]
    assert lib.nerf_grid_components_label(fake, C.byref(a)) == -1 and "reso[1]" in err()
    a.reso[:] = [1024, 1024, 1025]
    assert lib.nerf_grid_components_label(fake, C.byref(a)) == -1 and "reso[2]" in err()
    a.reso[:] = [4, 4, 4]
    a.struct_size += 8
    assert lib.nerf_grid_components_label(fake, C.byref(a)) == -1 and "struct_size" in err()

    count = C.c_int64(7)
    assert lib.nerf_grid_components_finish(None, fake, C.byref(count), None) == -1 and "NULL context" in err()
    assert lib.nerf_grid_components_finish(fake, None, C.byref(count), None) == -1 and "required" in err()
    assert lib.nerf_grid_components_finish(fake, fake, None, None) == -1 and "required" in err() and count.value == 7

    assert lib.nerf_grid_components_volumes(None, fake, 64, 3, fake, None) == -1 and "NULL context" in err()
    assert lib.nerf_grid_components_volumes(fake, fake, 0, 0, fake, None) == -1 and "n = 0" in err()
    assert lib.nerf_grid_components_volumes(fake, fake, 64, 65, fake, None) == -1 and "count = 65" in err()
    assert lib.nerf_grid_components_volumes(fake, None, 64, 3, fake, None) == -1 and "required" in err()
    assert lib.nerf_grid_components_volumes(fake, None, 64, 0, None, None) == 0      # no components: nothing is done

    assert lib.nerf_grid_components_keep(None, fake, fake, 64, fake, 3, fake, None) == -1 and "NULL context" in err()
    assert lib.nerf_grid_components_keep(fake, fake, fake, 64, None, 3, fake, None) == -1 and "required" in err()
    assert lib.nerf_grid_components_keep(fake, fake, None, 64, None, 0, fake, None) == -1 and "required" in err()
    assert lib.nerf_grid_components_keep(fake, fake, fake, (1 << 30) + 1, fake, 3, fake, None) == -1 and "n = " in err()

    r = _lib.GridCopyRowsArgs()
    r.reso[:] = [4, 4, 4]
    r.cols = 27
    assert lib.nerf_grid_copy_rows(None, C.byref(r)) == -1 and "NULL context" in err()
    assert lib.nerf_grid_copy_rows(fake, None) == -1 and "NULL" in err()
    assert lib.nerf_grid_copy_rows(fake, C.byref(r)) == 0      # no rows: nothing is done
    r.old_rows, r.new_rows = 5, 6
    assert lib.nerf_grid_copy_rows(fake, C.byref(r)) == -1 and "new_rows" in err()
    r.old_rows, r.new_rows = 1 << 31, 6      # a capacity may exceed the 64 nodes of the lattice, up to the ABI's 2^31 - 1 rows
    assert lib.nerf_grid_copy_rows(fake, C.byref(r)) == -1 and "old_rows" in err()
    r.old_rows, r.new_rows = 100, 65          # ... the new rows, one per kept node, may not
    assert lib.nerf_grid_copy_rows(fake, C.byref(r)) == -1 and "new_rows" in err()
    r.old_rows, r.new_rows = (1 << 31) - 1, 6
    assert lib.nerf_grid_copy_rows(fake, C.byref(r)) == -1 and "required" in err()
    r.old_rows = 10
    assert lib.nerf_grid_copy_rows(fake, C.byref(r)) == -1 and "required" in err()
    r.cols = 0
    assert lib.nerf_grid_copy_rows(fake, C.byref(r)) == -1 and "cols" in err()


def test_grid_components_kernels_generated_code(tmp_path):
    """No scratch, no inline assembly, no compare-and-swap, no float atomic: integer minimum and integer add only, and the
    only atomic that returns a value is the minimum of the union. At most 64 VGPRs: 8 waves per SIMD."""
    text, asm, build = compile_kernels_to_asm(tmp_path, "grid_components_kernels.hip")
    assert "grid_components_kernels.hip" in build.SOURCES and "grid_components_api.cpp" in build.SOURCES
    assert not re.search(r"\basm\b|__asm", text)
    assert "atomicCAS" not in text and "atomicExch" not in text and not re.search(r"atomic\w*\(\s*\(?\s*float", text)
    assert set(re.findall(r"\b(atomic[A-Z]\w*)\(", text)) == {"atomicMin", "atomicAdd"}
    kernels = re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M)
    names = ("grid_occupancy_kernel", "grid_label_init_kernel", "grid_label_merge_kernel", "grid_label_flatten_kernel",
             "grid_label_scan_kernel", "grid_label_rank_kernel", "grid_label_spread_kernel", "grid_label_volumes_kernel",
             "grid_keep_mask_kernel", "grid_row_sources_kernel", "grid_copy_rows_kernel")
    for name in names:
        assert sum(name in k for k in kernels) == 1, (name, kernels)
    assert len(kernels) == len(names), kernels
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)
    assert len(sizes) == len(kernels) and all(int(s) == 0 for s in sizes), sizes
    assert not re.search(r"\bscratch_(load|store)", asm)
    assert "cmpswap" not in asm
    atomics = re.findall(r"^\s*((?:global|flat|buffer|ds)_atomic\S*)([^\n]*)", asm, re.M)
    ops = {op for op, _ in atomics}
    assert ops == {"global_atomic_smin", "global_atomic_add"}, ops      # integer minimum and integer add, nothing else
    returning = [op for op, rest in atomics if re.search(r"\b(sc0|glc)\b", rest)]
    assert returning and set(returning) == {"global_atomic_smin"}, returning      # only the union reads what its atomic returns
    assert any(op == "global_atomic_smin" and not re.search(r"\b(sc0|glc)\b", rest) for op, rest in atomics)      # path halving
    assert not re.search(r"_atomic_\w*(f32|f64|f16|fadd|fmin|fmax)", asm)
    lds = dict(zip(kernels, (int(s) for s in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", asm))))
    assert all(v == 0 or re.search("flatten|scan|rank", k) for k, v in lds.items()), lds
    vgprs = [int(v) for v in re.findall(r"\.vgpr_count:\s*(\d+)", asm)]
    print("vgprs per kernel:", dict(zip(kernels, vgprs)))
    assert len(vgprs) == len(kernels) and max(vgprs) <= 64      # 8 waves per SIMD
