"""Palette-quantised colours without a GPU (include/nerf_mi355x.h, "Sparse voxel grid: palette-quantised colours"): the numpy
oracle's own invariants, the file layout, the refusals of the new C entries on a context that is never dereferenced, the
struct mirrors and the generated code of the render kernels."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_palette_oracle as PO  # noqa: E402
from grid_testlib import assert_structs_match_c_header, compile_kernels_to_asm  # noqa: E402

PALETTE_STRUCTS = {"nerf_grid_median_cut_args": "GridMedianCutArgs", "nerf_grid_palette_desc": "GridPaletteDesc"}
PALETTE_SYMBOLS = ("nerf_grid_median_cut_workspace", "nerf_grid_quantize_median_cut", "nerf_grid_create_palette")


def colours(m, seed, kind="normal"):
    """the inputs the GPU tests share with these: seeded, fp32 [m, 3]"""
    rng = np.random.default_rng(seed)
    if kind == "normal":
        return rng.normal(size=(m, 3)).astype(np.float32)
    if kind == "equal":
        return np.tile(np.array([[0.25, -1.5, 3.0]], np.float32), (m, 1))
    if kind == "duplicates":      # few distinct values on the widest axis: the stable order decides
        c = rng.integers(-2, 3, size=(m, 3)).astype(np.float32)
        c[:, 1] = rng.integers(-8, 9, size=m).astype(np.float32)
        return c
    if kind == "zeros":           # +-0.0 on the chosen axis among small values of both signs
        c = np.zeros((m, 3), np.float32)
        c[:, 0] = rng.choice(np.array([0.0, -0.0, 1e-3, -1e-3], np.float32), size=m)
        c[:, 1] = rng.choice(np.array([0.0, -0.0], np.float32), size=m)
        return c
    if kind == "extent_tie":      # axes 1 and 2 span exactly [-2, 2], axis 0 less: axis 1 is cut
        c = rng.uniform(-1, 1, size=(m, 3)).astype(np.float32)
        c[0, 1:], c[1, 1:] = (-2.0, 2.0), (2.0, -2.0)
        return c
    if kind == "lattice":         # multiples of 1/16 in [-4, 4]: many equal keys, and the mean of one or two is a half exactly
        return (rng.integers(-64, 65, size=(m, 3)) / 16.0).astype(np.float32)
    raise ValueError(kind)


# (m, bits, kind, seed) of every quantiser case the GPU test compares with the oracle. The seeds are chosen so that no palette
# entry's fp64 mean lies within 2^-20 (relative) of a rounding boundary - test_no_case_has_a_mean_near_a_rounding_boundary -
# so that the order of an fp64 sum, the one thing the rule leaves open, cannot decide a half on these inputs.
SMALL_M = (0, 1, 2, 3, 5, 255, 256, 257)
SEED_BUMP = {(3, 1): 1, (2, 8): 1, (255, 8): 2, (256, 8): 1}      # the first seed of 1000 bits + m + i that passes that test
CASES = ([(m, bits, "normal", 1000 * bits + m + SEED_BUMP.get((m, bits), 0)) for bits in (1, 4, 8) for m in SMALL_M] +
         [(m, 16, "lattice", m) for m in (65535, 65536, 65537, 70001)] +
         [(300, 4, "equal", 0), (1000, 6, "duplicates", 1), (1000, 5, "zeros", 2), (500, 3, "extent_tie", 3)])


def near_boundary(means, rel=2.0 ** -20):
    """where an fp64 mean lies within ``rel`` (relative) of a point at which its rounding to half changes"""
    means = np.asarray(means, np.float64)
    return PO.to_half(means * (1 - rel)) != PO.to_half(means * (1 + rel))


# ---- the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,bits", [(0, 1), (1, 4), (2, 1), (3, 4), (5, 8), (255, 4), (256, 8), (257, 8), (1000, 1), (70001, 16)])
def test_oracle_partitions_by_the_halving_rule(m, bits):
    c = colours(m, 100 + m + bits)
    palette, ids, means, boxes = PO.median_cut(c, bits, return_means=True)
    assert palette.shape == (1 << bits, 3) and palette.dtype == np.float16 and ids.shape == (m,) and ids.dtype == np.uint16
    sizes = PO.box_sizes(m, bits)
    assert sizes.sum() == m and sizes.max() - sizes.min() <= 1 and np.all(np.diff(sizes[::1 << (bits - 1)]) <= 0)
    assert np.array_equal(np.bincount(ids, minlength=1 << bits), sizes)       # a partition with the rule's sizes
    assert np.array_equal(np.sort(np.concatenate(boxes)) if m else np.zeros(0), np.arange(m))
    for j, members in enumerate(boxes):
        if len(members) == 0:
            assert not palette[j].any()
            continue
        lo, hi = c[members].min(axis=0), c[members].max(axis=0)
        # the mean lies in [lo, hi]; rounding to half moves it by at most half a half-ulp, and never past a half
        assert np.all(palette[j].astype(np.float32) >= PO.to_half(lo).astype(np.float32))
        assert np.all(palette[j].astype(np.float32) <= PO.to_half(hi).astype(np.float32))
    if m >= 65536 and bits == 16:
        assert ids.max() == 65535


_oracle_results = {}


def oracle_case(case):
    """``(colours, palette, ids, means)`` of a case of CASES, computed once for the CPU and the GPU tests of one process"""
    if case not in _oracle_results:
        m, bits, kind, seed = case
        c = colours(m, seed, kind)
        palette, ids, means, _ = PO.median_cut(c, bits, return_means=True)
        for a in (c, palette, ids, means):
            a.setflags(write=False)
        _oracle_results[case] = (c, palette, ids, means)
    return _oracle_results[case]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_no_case_has_a_mean_near_a_rounding_boundary(case):
    c, palette, ids, means = oracle_case(case)
    m, bits = case[:2]
    assert not near_boundary(means).any(), np.argwhere(near_boundary(means))[:5]
    assert np.array_equal(palette, PO.to_half(means)) and np.array_equal(np.bincount(ids, minlength=1 << bits), PO.box_sizes(m, bits))
    if m >= 65536:
        assert ids.max() == 65535
    if case[2] == "lattice":      # one or two members a box, values on a lattice of 2^-4: every mean is a half already
        assert PO.box_sizes(m, bits).max() <= 2 and np.array_equal(palette.astype(np.float64), means)


@pytest.mark.parametrize("m,bits", [(1, 1), (2, 1), (5, 4), (16, 4), (255, 8), (256, 8)])
def test_oracle_is_exact_when_every_box_has_one_member(m, bits):
    c = colours(m, 7 * m + bits)
    c[0, 0], c[m - 1, 2] = -0.0, 0.0
    palette, ids = PO.median_cut(c, bits)
    assert PO.box_sizes(m, bits).max() <= 1 and len(set(ids.tolist())) == m
    assert np.array_equal(palette[ids].view(np.uint16), c.astype(np.float16).view(np.uint16))      # the bits: -0.0 stays -0.0


def test_oracle_orders_ties_and_signed_zeros_and_breaks_extent_ties_low():
    # two members, equal on the cut axis: the stable sort keeps row order
    _, ids = PO.median_cut(np.array([[2, 0, 1], [2, 0, 1], [2, 0, 1]], np.float32), 1)
    assert ids.tolist() == [0, 0, 1]
    # -0.0 sorts before +0.0 although they compare equal
    _, ids = PO.median_cut(np.array([[0.0, 0, 0], [-0.0, 0, 0]], np.float32), 1)
    assert ids.tolist() == [1, 0]
    # equal extents on axes 0 and 1: axis 0 decides
    _, ids = PO.median_cut(np.array([[1, 0, 0], [0, 1, 0]], np.float32), 1)
    assert ids.tolist() == [1, 0]
    _, ids = PO.median_cut(colours(64, 3, "extent_tie"), 1)
    assert ids[0] == 0 and ids[1] == 1                       # cut on axis 1 (where row 0 is lowest), not on axis 2
    assert np.array_equal(PO.sort_key(np.array([-np.inf, -1, -0.0, 0.0, 1e-45, 1], np.float32)),
                          np.sort(PO.sort_key(np.array([-np.inf, -1, -0.0, 0.0, 1e-45, 1], np.float32))))
    with pytest.raises(ValueError):
        PO.median_cut(np.array([[0, np.nan, 0]], np.float32), 1)


def test_quantise_table_and_dequantise_are_inverse_where_exact():
    rng = np.random.default_rng(5)
    B, cap = 4, 12
    sh = rng.normal(size=(cap, 3 * B)).astype(np.float16).astype(np.float32)
    density = rng.uniform(0, 2, (cap, 1)).astype(np.float32)
    q = PO.quantise_table(sh, density, B, bits=4, retain=1)
    assert q["quant_colors"].shape == (3, 16, 3) and q["quant_map"].shape == (3, cap) and q["data_retained"].shape == (1, cap, 3)
    assert np.array_equal(PO.dequantise(q["quant_colors"], q["quant_map"], q["data_retained"]), sh)      # 12 <= 16 entries
    t = PO.quantise_table(sh, density, B, bits=4, retain=1, sigma_thresh=1.0)
    drop = density[:, 0] <= 1.0
    assert drop.any() and not drop.all()
    assert not t["density_data"][drop].any() and not t["quant_map"][:, drop].any() and not t["data_retained"][:, drop].any()
    assert np.array_equal(t["density_data"][~drop], density[~drop])
    back = PO.dequantise(t["quant_colors"], t["quant_map"], t["data_retained"])
    assert np.array_equal(back[~drop], sh[~drop])


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import nerf_projects_amd  # noqa: F401
    from nerf_projects_amd import _lib
    return _lib.load()


def err(lib):
    return lib.nerf_last_error().decode()


def test_palette_structs_match_a_c_compile_of_the_header(tmp_path):
    assert_structs_match_c_header(tmp_path, PALETTE_STRUCTS)


def test_workspace_query_needs_no_device(lib):
    from nerf_projects_amd import _lib
    for s in PALETTE_SYMBOLS:
        assert hasattr(lib, s) and s in _lib.EXPORTS, s
    for m in (0, 1, 257, 70001, 2 ** 31 - 1):
        for bits in (1, 8, 16):
            n = lib.nerf_grid_median_cut_workspace(m, bits)
            # two key and two member arrays, the extents of 2^(bits - 1) boxes, the sort's share
            assert n >= 24 * m + 24 * (1 << (bits - 1)) and n <= 33 * m + (4 << 20), (m, bits, n)
    assert lib.nerf_grid_median_cut_workspace(10, 16) >= lib.nerf_grid_median_cut_workspace(10, 1)
    for m, bits, word in ((-1, 8, "m = -1"), (2 ** 31, 8, "m = 2147483648"), (10, 0, "bits = 0"), (10, 17, "bits = 17")):
        assert lib.nerf_grid_median_cut_workspace(m, bits) == -1 and word in err(lib)


def test_quantize_checks_its_arguments_without_a_device(lib):
    from nerf_projects_amd import _lib
    fake_ctx, ptr = C.c_void_p(0x1000), 0x2000      # never dereferenced: every check comes before the first launch
    count = C.c_int64(-5)

    def args(**k):
        a = _lib.GridMedianCutArgs()
        a.m, a.bits, a.colors, a.ids, a.palette, a.workspace = 100, 8, ptr, ptr, ptr, 0x10000
        a.workspace_bytes = lib.nerf_grid_median_cut_workspace(100, 8)
        a.nonfinite = C.pointer(count)
        for name, v in k.items():
            setattr(a, name, v)
        return a

    call = lib.nerf_grid_quantize_median_cut
    assert call(None, C.byref(args())) == -1 and "NULL context" in err(lib)
    assert call(fake_ctx, None) == -1 and "nerf_grid_median_cut_args is NULL" in err(lib)
    a = args()
    a.struct_size -= 8
    assert call(fake_ctx, C.byref(a)) == -1 and "struct_size" in err(lib)
    assert call(fake_ctx, C.byref(args(m=-1))) == -1 and "m = -1" in err(lib)
    assert call(fake_ctx, C.byref(args(m=2 ** 31))) == -1 and "2^31" in err(lib)
    for bits in (0, 17, -3):
        assert call(fake_ctx, C.byref(args(bits=bits))) == -1 and f"bits = {bits}" in err(lib)
    for name in ("colors", "ids"):
        assert call(fake_ctx, C.byref(args(**{name: None}))) == -1 and "colors and ids" in err(lib)
    assert call(fake_ctx, C.byref(args(palette=None))) == -1 and "palette" in err(lib)
    assert call(fake_ctx, C.byref(args(nonfinite=None))) == -1 and "nonfinite" in err(lib)
    assert call(fake_ctx, C.byref(args(workspace=None))) == -1 and "workspace" in err(lib)
    assert call(fake_ctx, C.byref(args(workspace=0x10010))) == -1 and "aligned" in err(lib)
    short = args()
    short.workspace_bytes -= 1
    assert call(fake_ctx, C.byref(short)) == -1 and "bytes" in err(lib)
    assert count.value == -5      # refused before anything was written


def test_create_palette_checks_its_arguments_without_a_device(lib):
    from nerf_projects_amd import _lib
    fake_ctx, ptr = C.c_void_p(0x1000), 0x2000

    def desc(**k):
        d = _lib.GridPaletteDesc()
        d.reso[:] = [4, 4, 4]
        d.basis_dim, d.capacity, d.bits, d.retain = 9, 10, 8, 1
        d.radius[:] = [1.0, 1.0, 1.0]
        d.links, d.density_data, d.quant_map, d.quant_colors, d.data_retained = ptr, ptr, ptr, ptr, ptr
        for name, v in k.items():
            setattr(d, name, v)
        return d

    call = lib.nerf_grid_create_palette
    h = C.c_void_p(1)
    assert call(None, C.byref(desc()), C.byref(h)) == -1 and "NULL argument" in err(lib)
    assert call(fake_ctx, C.byref(desc()), None) == -1 and "NULL argument" in err(lib)
    assert call(fake_ctx, None, C.byref(h)) == -1 and "nerf_grid_palette_desc is NULL" in err(lib) and not h.value
    d = desc()
    d.struct_size += 8
    assert call(fake_ctx, C.byref(d), C.byref(h)) == -1 and "struct_size" in err(lib)
    assert call(fake_ctx, C.byref(desc(basis_dim=3)), C.byref(h)) == -1 and "basis_dim = 3" in err(lib)
    for bits in (0, 17):
        assert call(fake_ctx, C.byref(desc(bits=bits)), C.byref(h)) == -1 and f"bits = {bits}" in err(lib)
    for retain in (-1, 10):
        assert call(fake_ctx, C.byref(desc(retain=retain)), C.byref(h)) == -1 and f"retain = {retain}" in err(lib)
    d = desc()
    d.reso[1] = 1
    assert call(fake_ctx, C.byref(d), C.byref(h)) == -1 and "reso[1] = 1" in err(lib)
    d = desc()
    d.radius[2] = 0.0
    assert call(fake_ctx, C.byref(d), C.byref(h)) == -1 and "radius" in err(lib)
    for k in ("links", "density_data", "quant_map", "quant_colors", "data_retained"):
        assert call(fake_ctx, C.byref(desc(**{k: None})), C.byref(h)) == -1 and "required" in err(lib), k
    # ... but a table nothing would read may be NULL: these get past that check and stop at the next one
    assert call(fake_ctx, C.byref(desc(retain=0, data_retained=None, quant_map=ptr + 1)), C.byref(h)) == -1 and "aligned" in err(lib)
    assert call(fake_ctx, C.byref(desc(retain=9, quant_map=None, quant_colors=None, data_retained=ptr + 1)), C.byref(h)) == -1
    assert "aligned" in err(lib)
    assert call(fake_ctx, C.byref(desc(capacity=-2)), C.byref(h)) == -1 and "capacity = -2" in err(lib)
    assert not h.value


def test_python_refusals_need_no_device():
    import nerf_projects_amd as N
    with pytest.raises(TypeError, match="from_grid"):
        N.PaletteGrid()
    with pytest.raises(TypeError, match="SparseGrid"):
        N.PaletteGrid.from_grid(object())
    with pytest.raises(NotImplementedError, match="to_palette"):
        N.PaletteGrid.from_nerf(None, 0, 1, 8)
    assert N.PaletteGrid.is_palette and issubclass(N.PaletteGrid, N.SparseGrid) and not getattr(N.SparseGrid, "is_palette", False)
    assert not getattr(N.PaletteGrid, "is_half", False) and hasattr(N.SparseGrid, "to_palette")
    fake = N.PaletteGrid.__new__(N.PaletteGrid)      # no handle is ever made on these paths
    fake._handle_ptr = None
    for make in (N.GridTrainer, N.GridModule, lambda g: N.resample_grid(g, 8), N.remove_floaters):
        with pytest.raises(TypeError, match=r"PaletteGrid.*to_float\(\)"):
            make(fake)
    with pytest.raises(TypeError, match="BackgroundGrid"):
        N.BackgroundGrid.from_grid(fake, 4, 16)
    with pytest.raises(TypeError, match="to_float"):
        fake.sh_data
    with pytest.raises(TypeError, match="from_grid"):
        fake.sh_data = None
    with pytest.raises(TypeError, match="to_float"):
        N.PaletteGrid.from_grid(fake)
    import torch
    with pytest.raises(RuntimeError, match="CPU"):
        N.quantize_median_cut(torch.zeros(4, 3), 4)


# ---- the file -----------------------------------------------------------------------------------------------------------
def test_save_writes_the_reference_names_shapes_and_dtypes(tmp_path):
    """save() without a GPU: the object is assembled by hand from the oracle's quantisation (no handle is made on this path)."""
    import torch
    import nerf_projects_amd as N
    from nerf_projects_amd.grid import BASIS_TYPE_SH, RenderOptions
    rng = np.random.default_rng(1)
    B, cap, bits, retain = 4, 18, 3, 1
    links = np.full((4, 5, 6), -1, dtype=np.int32)
    links[1:3, 1:4, 2:5] = np.arange(18, dtype=np.int32).reshape(2, 3, 3)
    links[0, 0, 0] = -7
    sh = rng.normal(size=(cap, 3 * B)).astype(np.float32)
    density = rng.uniform(0, 9, (cap, 1)).astype(np.float32)
    q = PO.quantise_table(sh, density, B, bits, retain)
    g = N.PaletteGrid.__new__(N.PaletteGrid)
    g._handle_ptr = g._handle_key = None
    g.basis_type, g.basis_dim, g.bits, g.retain, g.capacity = BASIS_TYPE_SH, B, bits, retain, cap
    g.radius, g.center = torch.tensor([1.0, 2.0, 3.0]), torch.tensor([0.5, 0.0, -0.5])
    g.opt = RenderOptions()
    g._links, g._density = torch.from_numpy(links), torch.from_numpy(density)
    g._map = torch.from_numpy(np.ascontiguousarray(q["quant_map"].T))                        # the device layouts
    g._colors = torch.from_numpy(q["quant_colors"])
    g._retained = torch.from_numpy(np.ascontiguousarray(q["data_retained"].transpose(1, 0, 2)))
    assert g.sh_bytes == 2 * (cap * 3 + 3 * 8 * 3 + cap * 3) and g.bytes_resident == g.sh_bytes + 4 * links.size + 4 * cap
    for compress in (False, True):
        path = str(tmp_path / f"p{int(compress)}.npz")
        g.save(path, compress=compress)
        z = np.load(path)
        assert sorted(z.files) == ["basis_type", "center", "data_retained", "density_data", "links", "quant_colors", "quant_map",
                                   "radius"]
        assert z["quant_colors"].dtype == np.float16 and z["quant_colors"].shape == (B - retain, 1 << bits, 3)
        assert z["quant_map"].dtype == np.uint16 and z["quant_map"].shape == (B - retain, cap)
        assert z["data_retained"].dtype == np.float16 and z["data_retained"].shape == (retain, cap, 3)
        assert z["density_data"].dtype == np.float32 and z["links"].dtype == np.int32 and z["links"].min() == -1
        for k in ("quant_colors", "quant_map", "data_retained", "density_data"):
            assert np.array_equal(z[k], q[k]), k
        assert np.array_equal(z["radius"], g.radius.numpy()) and int(z["basis_type"]) == BASIS_TYPE_SH
        # every kept row's colour is a palette entry of its function, inside that function's range
        back = PO.dequantise(z["quant_colors"], z["quant_map"], z["data_retained"]).reshape(cap, 3, B)
        assert np.array_equal(back[:, :, 0], sh.reshape(cap, 3, B)[:, :, 0].astype(np.float16).astype(np.float32))
    # svox2's loader does not mistake the file for its own
    with pytest.raises(KeyError):
        N.SparseGrid.read_npz(path)
    with pytest.raises(ValueError, match="not a palette grid"):
        other = str(tmp_path / "plain.npz")
        np.savez(other, links=links, density_data=density, sh_data=sh.astype(np.float16))
        N.PaletteGrid.load(other)


# ---- generated code -----------------------------------------------------------------------------------------------------
def test_palette_kernels_use_no_scratch_and_no_lds(tmp_path):
    text, asm, _ = compile_kernels_to_asm(tmp_path, "grid_palette_kernels.hip")
    code = re.sub(r"//[^\n]*", "", text)
    assert not re.search(r"\basm\b|__asm", code)
    # no second march: the file shades, grid_device.h walks
    assert not re.search(r"\bwhile\b|\bgrid_march\b|\bskip_jump\b", code) and len(re.findall(r"\bmarch_colour<", code)) == 1
    kernels = re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M)
    render = [k for k in kernels if "grid_palette_render_kernel" in k]
    # basis_dim 9, 4, 1 x (image, skip, count); the sample kernel; the index check
    assert len(render) == 24 and len(kernels) == 26, kernels
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)
    assert len(sizes) == len(kernels) and all(int(s) == 0 for s in sizes), sizes
    assert not re.search(r"\bscratch_(load|store)", asm)
    lds = re.findall(r"\.group_segment_fixed_size:\s*(\d+)", asm)
    assert len(lds) == len(kernels) and all(int(s) == 0 for s in lds), lds
    vgprs = dict(zip(kernels, (int(v) for v in re.findall(r"\.vgpr_count:\s*(\d+)", asm))))
    print("vgprs per kernel:", vgprs)
    # recorded: 66 - 68 at basis_dim 9, 7 waves per SIMD; 72 registers are the most that keep 7
    assert len(vgprs) == 26 and max(vgprs[k] for k in render) <= 72, vgprs
