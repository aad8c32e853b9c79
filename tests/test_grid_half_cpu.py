"""Sparse voxel grid with half-precision colours (include/nerf_mi355x.h, "Sparse voxel grid: half-precision colours"), the
parts that need no GPU: the C ABI of the new entry points and their argument checks, the row lengths, the generated code of
the kernels, and the numpy statement of the pack that the GPU test compares the kernel with."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from grid_testlib import assert_structs_match_c_header, compile_kernels_to_asm  # noqa: E402
from test_grid_cpu import GRIDS, load_fixture  # noqa: E402

HALF_MAX = np.float32(65504.0)
ROW_HALFS = {9: 32, 4: 16, 1: 4}
CHANNEL_HALFS = {9: 10, 4: 4, 1: 1}
ROW_BYTES = {9: (64, 108), 4: (32, 48), 1: (8, 12)}      # packed, fp32


# ---- the oracle of the pack --------------------------------------------------------------------------------------------
def np_round_half(sh):
    """``(halves [rows, 3 B] float16, clamped)``: the clamp to +-65504 (NaN stays NaN), then numpy's IEEE conversion (round to
    nearest even, subnormals kept); ``clamped`` counts the entries the clamp changed."""
    sh = np.asarray(sh, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        clamped = int((np.abs(sh) > HALF_MAX).sum())
        return np.clip(sh, -HALF_MAX, HALF_MAX).astype(np.float16), clamped


def np_pack(sh, basis_dim):
    """``(packed [rows, row_halfs] uint16, clamped)``: :func:`np_round_half` laid out as the header states - channel c at slot
    ``c * S``, ``S`` = 10 / 4 / 1, every other slot zero."""
    h, clamped = np_round_half(sh)
    B, S = basis_dim, CHANNEL_HALFS[basis_dim]
    out = np.zeros((h.shape[0], ROW_HALFS[B]), dtype=np.uint16)
    for c in range(3):
        out[:, c * S:c * S + B] = h[:, c * B:(c + 1) * B].view(np.uint16)
    return out, clamped


def np_unpack(packed, basis_dim):
    B, S = basis_dim, CHANNEL_HALFS[basis_dim]
    return np.concatenate([packed[:, c * S:c * S + B] for c in range(3)], 1).view(np.float16).astype(np.float32)


def test_the_oracle_rounds_clamps_and_pads():
    x = np.array([[1e5, -1e5, 65504.0, -65504.0, 65519.9, 65520.0, 1e-7, 6e-8, -0.0, np.nan, 0.1, 2.9e-8]], np.float32)
    h, clamped = np_round_half(x)
    assert clamped == 4      # +-1e5, 65519.9, 65520
    assert h[0, :6].astype(np.float32).tolist() == [65504.0, -65504.0, 65504.0, -65504.0, 65504.0, 65504.0]
    assert h[0, 6] > 0 and h[0, 7] == np.float16(2.0 ** -24) and np.signbit(h[0, 8]) and h[0, 8] == 0 and np.isnan(h[0, 9])
    assert h[0, 11] == 0      # below half the smallest subnormal
    assert np.isfinite(h[0, :9]).all()
    p, _ = np_pack(x, 4)
    assert p.shape == (1, 16) and (p[:, 12:] == 0).all()
    assert np.array_equal(np_unpack(p, 4), h.astype(np.float32), equal_nan=True)
    p9, _ = np_pack(np.arange(27, dtype=np.float32)[None], 9)
    assert p9.shape == (1, 32) and (p9[0, [9, 19, 29, 30, 31]] == 0).all()
    assert np_unpack(p9, 9)[0].tolist() == list(range(27))
    p1, _ = np_pack(np.array([[1.0, 2.0, 3.0]], np.float32), 1)
    assert p1.shape == (1, 4) and p1[0, 3] == 0 and np_unpack(p1, 1)[0].tolist() == [1.0, 2.0, 3.0]


def test_the_fixture_grids_are_exactly_half_representable():
    z = load_fixture()
    for name in GRIDS:
        sh = z[f"{name}_sh"]
        assert np.array_equal(sh.astype(np.float16).astype(np.float32), sh), name


# ---- C ABI ------------------------------------------------------------------------------------------------------------
HALF_STRUCTS = {"nerf_grid_half_desc": "GridHalfDesc", "nerf_grid_pack_half_args": "GridPackHalfArgs"}
HALF_SYMBOLS = ("nerf_grid_half_row_halfs", "nerf_grid_pack_half", "nerf_grid_unpack_half", "nerf_grid_create_half")


@pytest.fixture(scope="module")
def lib():
    import nerf_projects_amd  # noqa: F401
    from nerf_projects_amd import _lib
    return _lib.load()


def err(lib):
    return lib.nerf_last_error().decode()


def test_half_structs_match_a_c_compile_of_the_header(tmp_path):
    seen = assert_structs_match_c_header(tmp_path, HALF_STRUCTS, extra_prints=[
        f'printf("lanes {k} %d\\n", NERF_GRID_HALF_LANES_{k});' for k in ("DEFAULT", "SINGLE", "PAIR")])
    from nerf_projects_amd import _lib
    assert seen["lanes"] == {"DEFAULT": _lib.NERF_GRID_HALF_LANES_DEFAULT, "SINGLE": _lib.NERF_GRID_HALF_LANES_SINGLE,
                             "PAIR": _lib.NERF_GRID_HALF_LANES_PAIR}


def test_row_lengths_and_bytes(lib):
    from nerf_projects_amd import _lib, grid_half
    for s in HALF_SYMBOLS:
        assert hasattr(lib, s) and s in _lib.EXPORTS, s
    for B, n in ROW_HALFS.items():
        assert lib.nerf_grid_half_row_halfs(B) == n == grid_half.row_halfs(B)
        assert (2 * n, 4 * 3 * B) == ROW_BYTES[B]
        assert 64 % (2 * n) == 0      # a row never straddles a 64-byte line
        assert CHANNEL_HALFS[B] % 2 == 0 or B == 1
    for B in (0, 2, 3, 16, -1):
        assert lib.nerf_grid_half_row_halfs(B) == -1 and "basis_dim" in err(lib)
        with pytest.raises(ValueError, match="basis_dim"):
            grid_half.row_halfs(B)


def test_pack_and_unpack_check_their_arguments_without_a_device(lib):
    from nerf_projects_amd import _lib
    fake_ctx, ptr = C.c_void_p(0x1000), 0x2000      # never dereferenced: every check comes before the first launch

    def args(**k):
        a = _lib.GridPackHalfArgs()
        a.basis_dim, a.capacity, a.row0, a.rows, a.sh_data, a.sh_half = 9, 100, 0, 100, ptr, ptr
        for name, v in k.items():
            setattr(a, name, v)
        return a

    assert lib.nerf_grid_pack_half(None, C.byref(args())) == -1 and "NULL context" in err(lib)
    assert lib.nerf_grid_pack_half(fake_ctx, None) == -1 and "nerf_grid_pack_half_args is NULL" in err(lib)
    a = args()
    a.struct_size -= 8
    assert lib.nerf_grid_pack_half(fake_ctx, C.byref(a)) == -1 and "struct_size" in err(lib)
    for B in (0, 2, 10):
        assert lib.nerf_grid_pack_half(fake_ctx, C.byref(args(basis_dim=B))) == -1 and f"basis_dim = {B}" in err(lib)
    assert lib.nerf_grid_pack_half(fake_ctx, C.byref(args(rows=-1))) == -1 and "rows = -1" in err(lib)
    assert lib.nerf_grid_pack_half(fake_ctx, C.byref(args(capacity=-1))) == -1 and "capacity = -1" in err(lib)
    for row0, rows in ((1, 100), (101, 0), (-1, 5), (0, 101), (2 ** 62, 2 ** 62)):
        assert lib.nerf_grid_pack_half(fake_ctx, C.byref(args(row0=row0, rows=rows))) == -1
        assert "row0 + rows" in err(lib) and "capacity = 100" in err(lib), err(lib)
    assert lib.nerf_grid_pack_half(fake_ctx, C.byref(args(sh_data=None))) == -1 and "sh_data is NULL" in err(lib)
    assert lib.nerf_grid_pack_half(fake_ctx, C.byref(args(sh_half=None))) == -1 and "sh_half is NULL" in err(lib)
    assert lib.nerf_grid_pack_half(fake_ctx, C.byref(args(sh_half=ptr + 2))) == -1 and "aligned" in err(lib)
    assert lib.nerf_grid_pack_half(fake_ctx, C.byref(args(rows=0, row0=100))) == 0      # nothing to do, nothing launched

    assert lib.nerf_grid_unpack_half(None, ptr, 1, 9, ptr, None) == -1 and "NULL context" in err(lib)
    assert lib.nerf_grid_unpack_half(fake_ctx, ptr, 1, 5, ptr, None) == -1 and "basis_dim = 5" in err(lib)
    assert lib.nerf_grid_unpack_half(fake_ctx, ptr, -1, 9, ptr, None) == -1 and "rows = -1" in err(lib)
    assert lib.nerf_grid_unpack_half(fake_ctx, None, 1, 9, ptr, None) == -1 and "sh_half is NULL" in err(lib)
    assert lib.nerf_grid_unpack_half(fake_ctx, ptr, 1, 9, None, None) == -1 and "sh_data is NULL" in err(lib)
    assert lib.nerf_grid_unpack_half(fake_ctx, None, 0, 9, None, None) == 0


def test_create_half_checks_its_arguments_without_a_device(lib):
    from nerf_projects_amd import _lib
    fake_ctx, ptr = C.c_void_p(0x1000), 0x2000

    def desc(**k):
        d = _lib.GridHalfDesc()
        d.reso[:] = [4, 4, 4]
        d.basis_dim, d.capacity = 9, 10
        d.radius[:] = [1.0, 1.0, 1.0]
        d.links, d.density_data, d.sh_half = ptr, ptr, ptr
        for name, v in k.items():
            setattr(d, name, v)
        return d

    h = C.c_void_p(1)
    assert lib.nerf_grid_create_half(None, C.byref(desc()), C.byref(h)) == -1 and "NULL argument" in err(lib)
    assert lib.nerf_grid_create_half(fake_ctx, C.byref(desc()), None) == -1 and "NULL argument" in err(lib)
    assert lib.nerf_grid_create_half(fake_ctx, None, C.byref(h)) == -1 and "nerf_grid_half_desc is NULL" in err(lib) and not h.value
    d = desc()
    d.struct_size += 8
    assert lib.nerf_grid_create_half(fake_ctx, C.byref(d), C.byref(h)) == -1 and "struct_size" in err(lib)
    assert lib.nerf_grid_create_half(fake_ctx, C.byref(desc(basis_dim=3)), C.byref(h)) == -1 and "basis_dim = 3" in err(lib)
    assert lib.nerf_grid_create_half(fake_ctx, C.byref(desc(lanes=3)), C.byref(h)) == -1 and "lanes = 3" in err(lib)
    d = desc()
    d.reso[1] = 1
    assert lib.nerf_grid_create_half(fake_ctx, C.byref(d), C.byref(h)) == -1 and "reso[1] = 1" in err(lib)
    d = desc()
    d.radius[2] = 0.0
    assert lib.nerf_grid_create_half(fake_ctx, C.byref(d), C.byref(h)) == -1 and "radius" in err(lib)
    for k in ("links", "density_data", "sh_half"):
        assert lib.nerf_grid_create_half(fake_ctx, C.byref(desc(**{k: None})), C.byref(h)) == -1
        assert "sh_half" in err(lib) and "required" in err(lib)
    assert lib.nerf_grid_create_half(fake_ctx, C.byref(desc(capacity=-2)), C.byref(h)) == -1 and "capacity = -2" in err(lib)
    assert lib.nerf_grid_create_half(fake_ctx, C.byref(desc(sh_half=ptr + 2)), C.byref(h)) == -1 and "aligned" in err(lib)
    assert not h.value


def test_python_refusals_need_no_device():
    import nerf_projects_amd as N
    with pytest.raises(TypeError, match="from_grid"):
        N.HalfGrid()
    with pytest.raises(TypeError, match="SparseGrid"):
        N.HalfGrid.from_grid(object())
    with pytest.raises(NotImplementedError, match="to_half"):
        N.HalfGrid.from_nerf(None, 0, 1, 8)
    assert N.HalfGrid.is_half and issubclass(N.HalfGrid, N.SparseGrid) and not getattr(N.SparseGrid, "is_half", False)
    fake = N.HalfGrid.__new__(N.HalfGrid)      # no handle is ever made on these paths
    fake._handle_ptr = None
    for make in (N.GridTrainer, N.GridModule, lambda g: N.resample_grid(g, 8), N.remove_floaters):
        with pytest.raises(TypeError, match=r"to_float\(\)"):
            make(fake)
    with pytest.raises(TypeError, match="to_float"):
        fake.sh_data
    with pytest.raises(TypeError, match="update_sh"):
        fake.sh_data = None


# ---- generated code ------------------------------------------------------------------------------------------------------
def test_half_kernels_use_no_scratch_and_keep_eight_waves(tmp_path):
    text, asm, _ = compile_kernels_to_asm(tmp_path, "grid_half_kernels.hip")
    code = re.sub(r"//[^\n]*", "", text)
    assert not re.search(r"\basm\b|__asm", code)
    # no second march: the file shades, grid_device.h walks
    assert not re.search(r"\bwhile\b|\bgrid_march\b|\bskip_jump\b", code) and len(re.findall(r"\bmarch_colour<", code)) == 2
    kernels = re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M)
    render = [k for k in kernels if "grid_half_render_kernel" in k]
    # basis_dim 9 and 4 in both mappings, basis_dim 1 in one: 5 x (image, skip, count)
    assert len(render) == 40 and len(kernels) == 43, kernels
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)
    assert len(sizes) == len(kernels) and all(int(s) == 0 for s in sizes), sizes
    assert not re.search(r"\bscratch_(load|store)", asm)
    lds = re.findall(r"\.group_segment_fixed_size:\s*(\d+)", asm)
    assert all(int(s) == 0 for s in lds), lds
    vgprs = dict(zip(kernels, (int(v) for v in re.findall(r"\.vgpr_count:\s*(\d+)", asm))))
    print("vgprs per kernel:", vgprs)
    # 8 waves per SIMD (<= 64 VGPRs) in every timed launch: template arguments <B, PAIR, IMAGE, SKIP, COUNT>, mangled
    # ILi9ELb1ELb0ELb1ELb0E...; the instrumented launches (COUNT) of the pair mapping at basis_dim 9 may take 7
    timed = [k for k in render if re.search(r"ILi\d+E(Lb[01]E){3}Lb0E", k)]
    assert len(timed) == 20 and max(vgprs[k] for k in timed) <= 64, {k: vgprs[k] for k in timed}
    assert max(vgprs[k] for k in render) <= 72
