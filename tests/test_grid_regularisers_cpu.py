"""The sparse voxel grid's regularisers as values, the parts that need no GPU: the fp32 restatements
(tests/grid_regularisers_oracle.py) against fp64 torch statements of the same sums, fp64 autograd against the restated
analytic gradients and against central finite differences, the C ABI of the five entry points on a fake handle, and the
signatures of the three GridModule methods. The cases (lattices, cell lists, rays) are built here once and shared with
tests/test_grid_regularisers.py."""
import ctypes as C
import functools
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_oracle as GO  # noqa: E402
import grid_regularisers_oracle as RO  # noqa: E402
from grid_testlib import assert_structs_match_c_header, compile_kernels_to_asm  # noqa: E402
from test_grid import random_grid, random_grid_with_faces  # noqa: E402
from test_grid_train import hostile_rays, mixed_rays  # noqa: E402

# ---- total variation: the cases ---------------------------------------------------------------------------------------
TV_LATTICES = ((5, 4, 3), (9, 8, 7), (6, 6, 6), (33, 33, 33))
# (target, start_dim, end_dim) at basis_dim 9: both tables and a column sub-range; basis_dim 1 once, on one lattice
TV_TARGETS = (("density", 0, 1), ("sh", 0, 27), ("sh", 3, 11))
TV_CASES = [(r, 9, t, a, b) for r in TV_LATTICES for t, a, b in TV_TARGETS] + [((9, 8, 7), 1, "sh", 0, 3)]
PLATEAU, ROW0, EMPTY = (2, 1, 1), (3, 2, 1), (1, 2, 1)


@functools.lru_cache(maxsize=None)
def tv_lattice(reso, basis_dim):
    """About half of the nodes kept ((33, 33, 33): all of them), rows in random order, with: the 8 corners kept, so every face
    holds kept nodes; node ROW0 interior, its link exactly row 0, its three forward neighbours kept; a plateau of equal
    values, PLATEAU and its six neighbours; node EMPTY empty (link -7) with its three forward neighbours kept; links < -1 at a
    third of the other empty nodes. Returns (grid, the row of PLATEAU). Read only."""
    rng = np.random.default_rng(1000 * basis_dim + sum(reso))
    kept = rng.random(reso) < (1.0 if reso[0] > 16 else 0.5)
    kept[::reso[0] - 1, ::reso[1] - 1, ::reso[2] - 1] = True
    plus = [PLATEAU] + [tuple(PLATEAU[k] + s * (k == ax) for k in range(3)) for ax in range(3) for s in (-1, 1)]
    for node in plus + [ROW0] + [tuple(p[k] + (k == ax) for k in range(3)) for p in (ROW0, EMPTY) for ax in range(3)]:
        kept[node] = True
    kept[EMPTY] = False
    n = int(kept.sum())
    links = np.full(reso, -1, dtype=np.int32)
    links[kept] = rng.permutation(n).astype(np.int32)
    other = tuple(np.argwhere(links == 0)[0])
    links[other], links[ROW0] = links[ROW0], 0
    low = (~kept) & (rng.random(reso) < 0.3)
    links[low] = rng.integers(-9, -1, int(low.sum())).astype(np.int32)
    links[EMPTY] = -7
    dens = rng.uniform(-2.0, 30.0, (n, 1)).astype(np.float32)
    sh = rng.normal(0.0, 0.7, (n, 3 * basis_dim)).astype(np.float32)
    rows = np.array([links[p] for p in plus])
    dens[rows], sh[rows] = 1.5, -0.25
    g = {"links": links, "density_data": dens, "sh_data": sh, "radius": np.ones(3, np.float32), "center": np.zeros(3, np.float32)}
    for face in (links[0], links[-1], links[:, 0], links[:, -1], links[:, :, 0], links[:, :, -1]):
        assert (face >= 0).any()
    assert links[ROW0] == 0 and (links < -1).any() and ROW0 not in plus and EMPTY not in plus
    for a in g.values():
        a.setflags(write=False)
    return g, int(links[PLATEAU])


@functools.lru_cache(maxsize=None)
def tv_cell_list(reso):
    """int64 [301]: random nodes, duplicates, the nodes of the far faces' corners, the entries -1 and X Y Z"""
    rng = np.random.default_rng(sum(reso) + 7)
    X, Y, Z = reso
    n = X * Y * Z
    far = [n - 1, (X - 1) * Y * Z, (Y - 1) * Z, Z - 1, ((X - 1) * Y + Y - 1) * Z]
    some = rng.integers(0, n, 284)
    cells = np.concatenate([some, far, [-1, n], some[:10]]).astype(np.int64)
    rng.shuffle(cells)
    assert len(cells) == 301 and len(cells) % 256
    cells.setflags(write=False)
    return cells


@functools.lru_cache(maxsize=None)
def tv_case(reso, basis_dim, target, d0, d1, listed):
    """(grid, plateau row, cells or None, restated value fp32, fp64 value, fp64 autograd gradient, restated gradient) for a
    cotangent of 1. Computed once, shared by the CPU and the GPU tests (read only)."""
    g, plateau = tv_lattice(reso, basis_dim)
    cells = tv_cell_list(reso) if listed else None
    v32 = RO.tv_value(g, target, d0, d1, cells)
    v64, g64 = RO.tv_autograd64(g, target, d0, d1, cells)
    g32 = RO.tv_grad(g, target, d0, d1, cells)
    for a in (g64, g32):
        a.setflags(write=False)
    return g, plateau, cells, v32, v64, g64, g32


@pytest.mark.parametrize("listed", [False, True])
@pytest.mark.parametrize("reso,basis_dim,target,d0,d1", TV_CASES)
def test_tv_restatement_against_the_fp64_statement(reso, basis_dim, target, d0, d1, listed):
    """Value: every term is positive and formed by at most eight fp32 roundings of 2^-24 each, the sum is fp64 and the final
    rounding adds 6e-8: 1e-6 of the value. Gradient: the bar of the existing TV-gradient tests, 1e-5 of the largest entry."""
    g, plateau, cells, v32, v64, g64, g32 = tv_case(reso, basis_dim, target, d0, d1, listed)
    print(f"tv {reso} B={basis_dim} {target}[{d0}:{d1}] {'list' if listed else 'dense'}: value {v64:.6g}, fp32 off by "
          f"{abs(float(v32) - v64) / v64:.2e}; gradient off by {np.abs(g32 - g64).max() / np.abs(g64).max():.2e} of the largest entry")
    assert v32.dtype == np.float32 and v64 > 0 and abs(float(v32) - v64) <= 1e-6 * v64
    big = np.abs(g64).max()
    assert big > 0 and np.abs(g32 - g64).max() <= 1e-5 * big
    out = np.ones(g64.shape[1], bool)
    out[d0:d1] = False
    assert not g64[:, out].any() and not g32[:, out].any()
    if not listed:      # every cell around the plateau's centre is covered: exactly nothing arrives there
        assert not g32[plateau].any() and not g64[plateau].any() and np.isfinite(g32).all()


def test_tv_conventions_of_the_restatement():
    g, _ = tv_lattice((5, 4, 3), 9)
    n = len(RO.dense_cells((5, 4, 3)))
    assert n == 4 * 3 * 2
    # the dense form is the list of its own cells; a duplicate counts twice; an outside entry stays in the divisor
    cells = RO.dense_cells((5, 4, 3))
    for target in ("density", "sh"):
        dense = RO.tv_value(g, target)
        assert RO.tv_value(g, target, cells=cells) == dense
        twice = RO.tv_value(g, target, cells=np.concatenate([cells, cells]))
        assert abs(float(twice) - float(dense)) <= 1e-7 * float(dense)
        padded = RO.tv_value(g, target, cells=np.concatenate([cells, [-1, 60, 10 ** 12]]))
        assert abs(float(padded) * (n + 3) / n - float(dense)) <= 1e-6 * float(dense)
        assert RO.tv_value(g, target, cells=np.zeros(0, np.int64)) == 0 and RO.tv_value(g, target, 1, 1) == 0
        assert not RO.tv_grad(g, target, cells=np.zeros(0, np.int64)).any()
    # with ignore_edge the cell whose link is row 0 contributes nothing, without it does; an empty cell always does
    row0 = np.array([np.ravel_multi_index(ROW0, (5, 4, 3))])
    empty = np.array([np.ravel_multi_index(EMPTY, (5, 4, 3))])
    assert RO.tv_value(g, "sh", cells=row0) == 0 and RO.tv_value(g, "density", cells=row0) > 0
    assert RO.tv_value(g, "sh", cells=empty) > 0 and RO.tv_value(g, "density", cells=empty) > 0
    # a cotangent scales the gradient
    a, b = RO.tv_grad(g, "sh", cotangent=3.0), RO.tv_grad(g, "sh")
    assert np.abs(a - 3.0 * b).max() <= 1e-6 * np.abs(a).max()


@pytest.mark.parametrize("target,d0,d1", TV_TARGETS)
def test_tv_fp64_autograd_against_central_finite_differences(target, d0, d1):
    """On the smallest lattice, every entry of 24 rows: h = 1e-5 on values of order 1. The truncation error is h^2 f''' / 6
    with f''' of sqrt(1e-5 + d^2) at most 1e5 s^3: 1e-6 s^3 against gradient entries of order s; the rounding error is
    1e-16 |value| / h = 1e-11. The bar is 1e-6 of the largest entry."""
    g, _ = tv_lattice((5, 4, 3), 9)
    for cells in (None, tv_cell_list((5, 4, 3))):
        tab = RO.tv_table(g, target)[0].astype(np.float64)
        _, grad = RO.tv_autograd64(g, target, d0, d1, cells, cotangent=0.7)
        rng = np.random.default_rng(3)
        rows = rng.choice(tab.shape[0], 24, replace=False)
        h, worst = 1e-5, 0.0
        for r in rows:
            for c in range(d0, d1):
                vals = []
                for sgn in (1.0, -1.0):
                    p = tab.copy()
                    p[r, c] += sgn * h
                    vals.append(0.7 * float(RO.tv_value64(g, target, torch.from_numpy(p), d0, d1, cells)))
                worst = max(worst, abs((vals[0] - vals[1]) / (2 * h) - grad[r, c]))
        print(f"tv {target}[{d0}:{d1}] finite differences: max {worst / np.abs(grad).max():.2e} of the largest entry")
        assert np.abs(grad).max() > 0 and worst <= 1e-6 * np.abs(grad).max()


# ---- the sparsity term: the cases --------------------------------------------------------------------------------------
SPARSITY_OPT = dict(step_size=0.5, sigma_thresh=5.0, stop_thresh=1e-2, near_clip=0.3)
SPARSITY_BATCHES = (1, 63, 64, 65, 257)


@functools.lru_cache(maxsize=None)
def sparsity_case(basis_dim):
    """(grid, origins [257, 3], dirs, restated s fp32, s64, shaded counts, fp64 autograd gradient, restated gradient,
    cotangent [257]): 249 mixed rays and the 8 hostile ones at the end, part of the samples below sigma_thresh, rays that stop,
    near_clip > 0; with skip data, which changes nothing. A prefix of the batch is a batch of its own. Read only."""
    rng = np.random.default_rng(40 + basis_dim)
    g = random_grid_with_faces(rng, (12, 11, 13), 9, keep=0.4) if basis_dim == 9 else random_grid(rng, (14, 12, 13), 1, keep=0.4)
    o, d = mixed_rays(rng, g, 249)
    ho, hd = hostile_rays(g)
    o, d = np.concatenate([o, ho]), np.concatenate([d, hd])
    cot = rng.normal(size=len(o)).astype(np.float32)
    s, s64, count, samples = RO.sparsity(g, o, d, skip=GO.skip_distances(g["links"]), **SPARSITY_OPT)
    plain = RO.sparsity(g, o, d, **SPARSITY_OPT)
    assert np.array_equal(plain[0], s) and np.array_equal(plain[2], count)
    _, g64 = RO.sparsity_autograd64(g, samples, cot, len(o))
    g32 = RO.sparsity_grad(g, samples, cot)
    for a in (o, d, cot, s, s64, count, g64, g32):
        a.setflags(write=False)
    return g, o, d, s, s64, count, g64, g32, cot, samples


@pytest.mark.parametrize("basis_dim", [9, 1])
def test_sparsity_restatement_against_the_fp64_statement(basis_dim):
    """Value per ray: one rounding per accumulation plus the few of a term, (n_r + 16) 2^-24 of the value. Gradient: 1e-5 of
    the largest entry."""
    g, o, d, s, s64, count, g64, g32, cot, samples = sparsity_case(basis_dim)
    stat64, _ = RO.sparsity_autograd64(g, samples, cot, len(o))
    assert np.abs(stat64 - s64).max() <= 1e-5 * s64.max()      # the fp64 statement (fp64 interpolation) and the fp64 sum of the fp32 sigmas
    assert (np.abs(s.astype(np.float64) - s64) <= (count + 16) * 2.0 ** -24 * s64).all()
    assert (count > 0).sum() > 150 and not s[-8:].any() and not count[-8:].any()      # hostile rays: exactly 0
    full = RO.sparsity(g, o, d, **dict(SPARSITY_OPT, sigma_thresh=0.0, stop_thresh=0.0))
    assert (full[2] > count).sum() > 100      # the thresholds bite: samples below sigma_thresh, rays that stop early
    big = np.abs(g64).max()
    print(f"sparsity B={basis_dim}: gradient restatement vs fp64 autograd {np.abs(g32 - g64).max() / big:.2e} of the largest entry")
    assert big > 0 and np.abs(g32 - g64).max() <= 1e-5 * big


def test_sparsity_fp64_autograd_against_central_finite_differences():
    """Over the fixed sample set the sum is smooth: log1p(2 sigma^2) with sigma linear in the densities. h = 1e-4 on densities
    of order 10: truncation h^2 f''' / 6 <= 1e-8, rounding 1e-16 |s| / h = 1e-9 of entries of order 1. Bar: 1e-6 of the largest."""
    g, o, d, _, _, _, g64, _, cot, samples = sparsity_case(1)
    dens = g["density_data"].astype(np.float64)
    rows = np.argsort(-np.abs(g64[:, 0]))[:30]
    w = torch.from_numpy(cot.astype(np.float64))
    h, worst = 1e-4, 0.0
    for r in rows:
        vals = []
        for sgn in (1.0, -1.0):
            p = dens.copy()
            p[r, 0] += sgn * h
            vals.append(float((w * RO.sparsity64(g, samples, torch.from_numpy(p), len(o))).sum()))
        worst = max(worst, abs((vals[0] - vals[1]) / (2 * h) - g64[r, 0]))
    print(f"sparsity finite differences: max {worst / np.abs(g64).max():.2e} of the largest entry")
    assert worst <= 1e-6 * np.abs(g64).max()


# ---- C ABI ------------------------------------------------------------------------------------------------------------
NEW_STRUCTS = {"nerf_grid_tv_value_args": "GridTvValueArgs", "nerf_grid_sparsity_args": "GridSparsityArgs"}
NEW_SYMBOLS = ("nerf_grid_tv_value_workspace", "nerf_grid_tv_value", "nerf_grid_tv_value_backward", "nerf_grid_sparsity_rays",
               "nerf_grid_sparsity_backward")


def test_regulariser_structs_and_constants_match_a_c_compile_of_the_header(tmp_path):
    import nerf_projects_amd  # noqa: F401
    from nerf_projects_amd import _lib
    consts = assert_structs_match_c_header(tmp_path, NEW_STRUCTS, extra_prints=[
        'printf("consts tv %d\\n", NERF_GRID_TV_DENSITY * 10 + NERF_GRID_TV_SH);'])
    assert consts == {"consts": {"tv": _lib.NERF_GRID_TV_DENSITY * 10 + _lib.NERF_GRID_TV_SH}}


def test_tv_value_workspace():
    """one fp64 partial per workgroup of 256 items; 64-bit: 2^30 nodes times 27 columns pass 2^32"""
    import nerf_projects_amd  # noqa: F401
    from nerf_projects_amd import _lib
    ws = _lib.load().nerf_grid_tv_value_workspace
    assert [ws(n) for n in (-1, 0, 1, 255, 256, 257)] == [0, 0, 1, 1, 1, 2]
    assert ws((1 << 30) * 27) == (1 << 22) * 27 and ws((1 << 30) * 27 + 1) == (1 << 22) * 27 + 1


def test_regulariser_calls_refuse_bad_arguments_before_any_device_call():
    """Every refusal here comes before the handle is dereferenced or a kernel launched: the pointers are fakes."""
    import nerf_projects_amd  # noqa: F401
    from nerf_projects_amd import _lib
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in _lib.EXPORTS
    fake = C.c_void_p(0x1000)
    err = lambda: lib.nerf_last_error().decode()      # noqa: E731

    def tv(**kw):
        a = _lib.GridTvValueArgs()
        a.target, a.start_dim, a.end_dim, a.ignore_edge = _lib.NERF_GRID_TV_SH, 0, 3, 1
        a.cells = a.partials = a.value = a.grad_value = a.grad = 0x1000
        a.n_cells = 5
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for fn, name, own in ((lib.nerf_grid_tv_value, NEW_SYMBOLS[1], (({"value": 0}, "value is NULL"),)),
                          (lib.nerf_grid_tv_value_backward, NEW_SYMBOLS[2], (({"grad_value": 0}, "grad_value and grad"),
                                                                              ({"grad": 0}, "grad_value and grad")))):
        assert fn(None, C.byref(tv())) == -1 and "NULL grid" in err()
        assert fn(fake, None) == -1 and "NULL" in err()
        cases = [({"target": 2}, "target"), ({"target": -1}, "target"), ({"ignore_edge": 2}, "ignore_edge"),
                 ({"cells_int64": 2}, "cells_int64"), ({"n_cells": -1}, "n_cells"), ({"n_cells": (1 << 30) + 1}, "n_cells"),
                 ({"start_dim": -1}, "columns"), ({"start_dim": 4}, "columns"),
                 ({"target": _lib.NERF_GRID_TV_DENSITY, "end_dim": 2}, "columns")] + list(own)
        for kw, word in cases:
            assert fn(fake, C.byref(tv(**kw))) == -1 and word in err() and name + ":" in err(), (name, kw, err())
        for delta in (-8, 8):
            a = tv()
            a.struct_size += delta
            assert fn(fake, C.byref(a)) == -1 and "struct_size" in err()

    def options():
        opt = _lib.GridRenderOptions()
        opt.step_size, opt.sigma_thresh, opt.stop_thresh, opt.background_brightness = 0.5, 1e-10, 1e-7, 1.0
        return opt

    def rays(**kw):
        a = _lib.GridSparsityArgs()
        a.origins = a.dirs = a.sparsity = a.grad_sparsity = a.grad_density = 0x1000
        a.n_rays = 5
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for fn, name, own in ((lib.nerf_grid_sparsity_rays, NEW_SYMBOLS[3], (({"sparsity": 0}, "sparsity is NULL"),)),
                          (lib.nerf_grid_sparsity_backward, NEW_SYMBOLS[4], (({"grad_sparsity": 0}, "grad_sparsity and grad_density"),
                                                                              ({"grad_density": 0}, "grad_sparsity and grad_density")))):
        assert fn(None, C.byref(options()), C.byref(rays())) == -1 and "NULL grid" in err()
        assert fn(fake, C.byref(options()), None) == -1 and "NULL" in err()
        assert fn(fake, None, C.byref(rays())) == -1 and "NULL" in err()
        for delta in (-8, 8):
            a = rays()
            a.struct_size += delta
            assert fn(fake, C.byref(options()), C.byref(a)) == -1 and "struct_size" in err()
        for field in ("last_sample_opaque", "randomize"):
            opt = options()
            setattr(opt, field, 1)
            assert fn(fake, C.byref(opt), C.byref(rays())) == -1 and field in err() and "not built" in err()
        opt = options()
        opt.step_size = 0.0
        assert fn(fake, C.byref(opt), C.byref(rays())) == -1 and "step_size" in err()
        for kw, word in [({"n_rays": -1}, "n_rays"), ({"n_rays": (1 << 26) + 1}, "n_rays"), ({"origins": 0}, "n_rays"),
                         ({"dirs": 0}, "n_rays")] + list(own):
            assert fn(fake, C.byref(options()), C.byref(rays(**kw))) == -1 and word in err() and name + ":" in err(), (name, kw, err())
        assert fn(fake, C.byref(options()), C.byref(rays(n_rays=0, sparsity=0, grad_sparsity=0))) == 0      # zero rays: nothing is done


def test_module_methods_exist_with_their_signatures():
    import nerf_projects_amd as N
    from nerf_projects_amd import grid_autograd
    sig = {name: list(inspect.signature(getattr(N.GridModule, name)).parameters.items()) for name in ("tv", "tv_color", "sparsity_loss")}
    assert [(k, p.default) for k, p in sig["tv"][:2]] == [("self", inspect.Parameter.empty), ("cells", None)]
    assert [(k, p.default) for k, p in sig["tv_color"][1:4]] == [("start_dim", 0), ("end_dim", None), ("cells", None)]
    assert [k for k, _ in sig["sparsity_loss"]] == ["self", "rays"]
    for name in ("tv", "tv_color"):
        names = [k for k, _ in sig[name]]
        assert "logalpha" in names and "ndc_coeffs" in names
        assert "ndc_coeffs" in getattr(N.GridModule, name).__doc__
    m = N.GridModule.__new__(N.GridModule)
    with pytest.raises(NotImplementedError, match="logalpha"):
        m.tv(logalpha=True)
    with pytest.raises(NotImplementedError, match="logalpha"):
        m.tv_color(logalpha=True)
    with pytest.raises(RuntimeError, match="CPU"):
        grid_autograd._cells_arg(torch.zeros(4, dtype=torch.int64), torch.device("cuda"))
    with pytest.raises(TypeError, match="int32 or int64"):
        grid_autograd._cells_arg(torch.zeros(4), torch.device("cuda"))
    doc = grid_autograd.__doc__
    assert "tv_color" in doc and "sparsity_loss" in doc
    # SparseGrid's own svox2-named methods keep raising
    for name in ("tv", "tv_color"):
        with pytest.raises(NotImplementedError):
            getattr(N.SparseGrid, name)(N.SparseGrid.__new__(N.SparseGrid))


def test_grid_regularisers_kernels_generated_code(tmp_path):
    """No scratch, no inline assembly, no compare-and-swap: every float add is one hardware atomic without return, and the
    value is summed without any float atomic (LDS only in the two kernels of the sum). The device functions of the march are
    grid_device.h's, used and not copied."""
    text, asm, build = compile_kernels_to_asm(tmp_path, "grid_regularisers_kernels.hip")
    assert "grid_regularisers_kernels.hip" in build.SOURCES and "grid_regularisers_api.cpp" in build.SOURCES
    assert not re.search(r"\basm\b|__asm", text)
    text += open(os.path.join(build.CSRC, "grid_regularisers_device.h")).read()      # the two ray kernels are written there
    for fn in ("setup_ray", "grid_march", "corner_weight", "node_to_xyz"):
        assert re.search(r"\b%s\b" % fn, text) and not re.search(r"\b(void|float|int)\s+%s\b" % fn, text), fn
    kernels = re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M)
    assert len(kernels) == 7, kernels      # value, finish, backward; sparsity and its backward with and without skip data
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)
    assert len(sizes) == len(kernels) and all(int(s) == 0 for s in sizes), sizes
    lds = dict(zip(kernels, (int(s) for s in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", asm))))
    assert sorted(v for v in lds.values() if v) == [256 * 8, 1024 * 8], lds
    assert all(("tv_value_kernel" in k or "finish" in k) == bool(v) for k, v in lds.items()), lds
    assert not re.search(r"\bscratch_(load|store)", asm) and "cmpswap" not in asm
    assert len(re.findall(r"\bglobal_atomic_add_f32\b", asm)) == 4 + 2 * 8      # 4 nodes of a cell; 8 corners, two kernels
    assert not re.search(r"global_atomic_add_f32[^\n]*\bsc0\b", asm)      # none returns the old value
    vgprs = dict(zip(kernels, (int(v) for v in re.findall(r"\.vgpr_count:\s*(\d+)", asm))))
    print("vgprs per kernel:", vgprs)
    assert max(vgprs.values()) <= 64
