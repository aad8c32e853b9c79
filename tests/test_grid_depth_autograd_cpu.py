"""Gradients of the sparse voxel grid's expected depth and log_transmit, the parts that need no GPU: the numpy restatement
(tests/grid_depth_autograd_oracle.py) against the gradients recorded from the reference's renderer under torch autograd
(tests/golden/grid_depth_autograd.npz), against central finite differences of its own forward and against the depth oracle,
the C ABI of the two entry points, what the module refuses, and the generated code of csrc/grid_depth_autograd_kernels.hip."""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_depth_autograd_oracle as DA  # noqa: E402
import grid_depth_oracle as DO  # noqa: E402
import grid_oracle as GO  # noqa: E402
from grid_testlib import assert_structs_match_c_header, compile_kernels_to_asm  # noqa: E402

RENDER = os.path.join(ROOT, "tests", "golden", "grid_render.npz")
DEPTH = os.path.join(ROOT, "tests", "golden", "grid_depth.npz")
FIXTURE = os.path.join(ROOT, "tests", "golden", "grid_depth_autograd.npz")
GOLDEN_E = ("i", "ii", "iii")


def sparse_grids():
    """the sparse grids of golden (iv) that the generator kept (inside its cap)"""
    a = np.load(FIXTURE)
    return tuple(n for n in ("a", "b", "c") if f"{n}_iv_grad64" in a.files)


def fixture_grid(name):
    z = np.load(DEPTH if name == "e" else RENDER)
    return ({"links": z[f"{name}_links"], "density_data": z[f"{name}_density"], "sh_data": z[f"{name}_sh"],
             "radius": z[f"{name}_radius"], "center": z[f"{name}_center"]}, z[f"{name}_origins"], z[f"{name}_dirs"])


def grad_bar(a, prefix):
    """(fp64 gradient, bar): 3x the reference's own fp32 - fp64 distance, and no tighter than 1e-5 of the largest entry"""
    want = a[prefix + "_grad64"].astype(np.float64)
    return want, max(3.0 * float(a[prefix + "_d_ref"]), 1e-5 * float(np.abs(want).max()))


def golden_loss(a, name, kind, depth, log_t):
    """The loss of golden ``kind`` as torch code on ``depth`` and ``log_transmit`` (tensors of any device and precision): the
    reference's T is exp(log_transmit)."""
    T = torch.exp(log_t)
    as_t = lambda x: torch.from_numpy(x).to(device=depth.device, dtype=depth.dtype)      # noqa: E731
    if kind == "i":
        return (as_t(a["e_w"]) * depth).sum()
    if kind == "ii":
        return (as_t(a["e_w2"]) * T).sum()
    if kind == "iii":
        eps = float(a["eps"])
        return ((depth / (1.0 - T + eps) - 1.0) ** 2).mean() + 0.1 * (T * (1.0 - T)).mean()
    assert kind == "iv"
    return (as_t(a[f"{name}_w2"]) * T).sum()


def golden_cotangents(a, name, kind, depth, log_t):
    """d loss / d depth and d loss / d log_transmit of :func:`golden_loss` at numpy ``depth``, ``log_t``, in their precision
    (None where the loss does not use that output)"""
    dt, lt = (torch.from_numpy(np.array(x)).requires_grad_(True) for x in (depth, log_t))
    golden_loss(a, name, kind, dt, lt).backward()
    return tuple(None if t.grad is None else t.grad.numpy() for t in (dt, lt))


@functools.lru_cache(maxsize=None)
def oracle_golden_case(name, kind, dtype):
    """grad_density of the restatement for a golden loss at the PyTorch renderer's setting (sigma_thresh = 0,
    stop_thresh = 0); computed once, read only"""
    a = np.load(FIXTURE)
    g, o, d = fixture_grid(name)
    kw = dict(sigma_thresh=0.0, stop_thresh=0.0, dtype=dtype)
    depth, log_t, tape = DA.depth_taped(g, o, d, **kw)
    g_d, g_t = golden_cotangents(a, name, kind, depth, log_t)
    gd = DA.depth_backward(g, o, d, g_d, g_t, None if g_d is None else tape, **kw)
    gd.setflags(write=False)
    return gd


def golden_cases():
    return [("e", k) for k in GOLDEN_E] + [(n, "iv") for n in sparse_grids()]


def test_fixture_holds_arrays_only_is_small_and_inside_its_cap():
    assert os.path.getsize(FIXTURE) < 1 << 20
    a = np.load(FIXTURE)      # (allow_pickle is off: arrays only)
    ze = np.load(DEPTH)
    kept = sparse_grids()
    assert len(kept) >= 1      # grid e and at least one sparse grid
    want = {"e_w", "e_w2", "eps"} | {f"{n}_w2" for n in kept}
    for name, kind in golden_cases():
        prefix = f"{name}_{kind}"
        want |= {prefix + "_grad64", prefix + "_d_ref"}
        g64, d_ref = a[prefix + "_grad64"], float(a[prefix + "_d_ref"])
        cap = fixture_grid(name)[0]["density_data"].shape
        assert g64.shape == cap and g64.dtype == np.float32 and a[prefix + "_d_ref"].dtype == np.float64
        big = float(np.abs(g64).max())
        print(f"golden ({kind}) grid {name}: d_ref / max |g64| = {d_ref / big:.2e}")
        assert 0 < 3.0 * d_ref <= 1e-2 * big      # the bar max(3 d_ref, ...) is at most 1 % of the largest entry
    assert set(a.files) == want
    assert a["e_w"].shape == a["e_w2"].shape == (len(ze["e_origins"]),) and float(a["eps"]) == 1e-3


@pytest.mark.parametrize("name,kind", golden_cases())
def test_fp64_restatement_matches_the_reference_autograd(name, kind):
    a = np.load(FIXTURE)
    got = oracle_golden_case(name, kind, np.float64)
    want, tol = grad_bar(a, f"{name}_{kind}")
    err = np.abs(got - want)
    print(f"golden ({kind}) grid {name}: fp64 restatement vs fp64 autograd max {err.max():.3e} (bar {tol:.3e}, max |g| {np.abs(want).max():.3e})")
    assert got.dtype == np.float64 and err.max() <= tol, (name, kind, int(err.argmax()), err.max(), tol)      # every entry


@pytest.mark.parametrize("name,kind", golden_cases())
def test_fp32_restatement_matches_the_reference_autograd(name, kind):
    """the form the kernel is held to on the GPU, against the same bar"""
    a = np.load(FIXTURE)
    got = oracle_golden_case(name, kind, np.float32)
    want, tol = grad_bar(a, f"{name}_{kind}")
    err = np.abs(got.astype(np.float64) - want)
    print(f"golden ({kind}) grid {name}: fp32 restatement vs fp64 autograd max {err.max():.3e} (bar {tol:.3e})")
    assert got.dtype == np.float32 and err.max() <= tol, (name, kind, int(err.argmax()), err.max(), tol)


def small_grid(seed=21):
    """6 x 5 x 7, every node kept but the 8 corners of two cells, rows in random order, every density positive (the gate
    sigma > sigma_thresh = 0 is then decided by the links alone: the forward is smooth in the densities)"""
    rng = np.random.default_rng(seed)
    reso = (6, 5, 7)
    kept = np.ones(reso, dtype=bool)
    kept[:2, :2, :2] = False
    kept[3:5, 2:4, 4:6] = False
    n = int(kept.sum())
    links = np.full(reso, -1, dtype=np.int32)
    links[kept] = rng.permutation(n).astype(np.int32)
    g = {"links": links, "density_data": rng.uniform(0.25, 4.0, (n, 1)).astype(np.float32),
         "sh_data": np.zeros((n, 3), np.float32), "radius": np.array([1.0, 1.2, 0.9], np.float32),
         "center": np.array([0.1, 0.0, -0.1], np.float32)}
    u = rng.normal(size=(64, 3))
    o = (g["center"] + 3.0 * g["radius"] * u / np.linalg.norm(u, axis=-1, keepdims=True)).astype(np.float32)
    d = (g["center"] + g["radius"] * rng.uniform(-0.8, 0.8, (64, 3)) - o).astype(np.float32)
    return g, o, d, rng


def test_fp64_restatement_is_the_derivative_of_its_own_forward():
    """Central finite differences of L = sum(w depth) + sum(w2 log_T) in fp64 on 40 rows, each cotangent alone and both.
    With h = 1e-4 on densities of order 1 the truncation error is h^2 L''' / 6 ~ 1e-8 of a gradient entry and the rounding
    error 1e-16 |L| / h ~ 1e-11: the bar is 1e-6 of the largest entry."""
    g, o, d, rng = small_grid()
    w, w2 = rng.normal(size=64), rng.normal(size=64)
    dens = g["density_data"].astype(np.float64)
    kw = dict(sigma_thresh=0.0, stop_thresh=0.0, dtype=np.float64)
    depth, log_t, tape = DA.depth_taped(g, o, d, density=dens, **kw)
    assert (depth > 0).sum() > 40 and np.array_equal(tape, depth)
    rows = rng.choice(dens.shape[0], 40, replace=False)
    h = 1e-4
    fd = np.zeros((40, 2))
    for i, r in enumerate(rows):
        vals = []
        for sgn in (1.0, -1.0):
            p = dens.copy()
            p[r, 0] += sgn * h
            dp, lp, _ = DA.depth_taped(g, o, d, density=p, **kw)
            vals.append(((w * dp).sum(), (w2 * lp).sum()))
        fd[i] = [(vals[0][k] - vals[1][k]) / (2 * h) for k in (0, 1)]
    gd_d = DA.depth_backward(g, o, d, w, None, tape, density=dens, **kw)
    gd_t = DA.depth_backward(g, o, d, None, w2, None, density=dens, **kw)
    gd_b = DA.depth_backward(g, o, d, w, w2, tape, density=dens, **kw)
    for label, got, want in (("depth", gd_d, fd[:, 0]), ("log_T", gd_t, fd[:, 1]), ("both", gd_b, fd.sum(-1))):
        big = np.abs(got).max()
        err = np.abs(got[rows, 0] - want).max()
        print(f"finite differences, {label} cotangent: max {err:.3e} = {err / big:.2e} of the largest entry")
        assert (want != 0).sum() >= 30 and err <= 1e-6 * big, label
    assert np.abs(gd_b - (gd_d + gd_t)).max() <= 1e-12 * np.abs(gd_b).max()


def test_fp32_restatement_against_its_fp64_form():
    """The two forms differ by the fp32 roundings of the values (the lattice is shared). log_T is a sum of up to ~40 terms
    each rounded to 2^-24 of a partial sum that matters only while |log_T| < 16 (T > 1e-7): an absolute 40 x 16 x 6e-8 =
    4e-5 in log_T, so a relative 4e-5 in T and in every weight; lead - remaining subtracts two such values of the size of
    the depth whose difference may be a tenth of it. A gradient entry therefore carries a few 1e-4 of the largest: the bar
    is 1e-3 of it. The direct log_T cotangent involves no exponential at all (d_sigma = -g_T step_ds): 1e-5."""
    g, o, d = fixture_grid("e")
    a = np.load(FIXTURE)
    for label, g_d, g_t, rel in (("depth", a["e_w"], None, 1e-3), ("log_T", None, a["e_w2"], 1e-5), ("both", a["e_w"], a["e_w2"], 1e-3)):
        got = DA.depth_vjp(g, o, d, g_d, g_t)[2]
        want = DA.depth_vjp(g, o, d, g_d, g_t, dtype=np.float64)[2]
        big, err = np.abs(want).max(), np.abs(got.astype(np.float64) - want).max()
        print(f"fp32 vs fp64 restatement, {label} cotangent: max {err:.3e} = {err / big:.2e} of the largest entry (bar {rel:.0e})")
        assert got.dtype == np.float32 and want.dtype == np.float64 and big > 0 and err <= rel * big, label


@pytest.mark.parametrize("name", ("a", "c", "e"))
def test_taped_forward_is_the_depth_oracle_bit_for_bit(name):
    """depth and log_transmit are grid_depth_oracle's (which is pinned to the reference), with and without skip data and at
    off-default options with rays that stop; the tape is the fp64 sum of the fp32 terms, so it rounds to within a few
    ulps of the fp32 sum."""
    g, o, d = fixture_grid(name)
    skip = GO.skip_distances(g["links"])
    for kw in ({}, {"sigma_thresh": 0.0, "stop_thresh": 0.0}, {"near_clip": 2.0, "step_size": 0.3, "sigma_thresh": 0.5, "stop_thresh": 1e-2}):
        want = DO.depth(g, o, d, **kw)
        for sk in (None, skip):
            depth, log_t, tape = DA.depth_taped(g, o, d, skip=sk, **kw)
            assert np.array_equal(depth, want[0]) and np.array_equal(log_t, want[1]), (name, kw)
            assert tape.dtype == np.float64 and np.abs(tape - depth).max() <= 1e-5 * max(depth.max(), 1.0)
            assert np.array_equal(tape == 0, depth == 0)
    assert (DO.depth(g, o, d, near_clip=2.0, step_size=0.3, sigma_thresh=0.5, stop_thresh=1e-2)[1] == np.float32(-1e3)).any()


def test_stopped_rays_and_misses_in_the_restatement():
    """A ray that stops takes no log_T gradient and its depth gradient ends at the stopping sample; skip data changes the
    gradient by nothing but the rounding of nothing (the same samples in the same order: equal bits)."""
    g, o, d = fixture_grid("e")
    n = len(o)
    kw = dict(stop_thresh=1e-2)
    depth, log_t, tape = DA.depth_taped(g, o, d, **kw)
    stopped = log_t == np.float32(-1e3)
    assert 50 < stopped.sum() < n - 50
    ones = np.ones(n, np.float32)
    gt_all = DA.depth_backward(g, o, d, None, ones, None, **kw)
    gt_live = DA.depth_backward(g, o[~stopped], d[~stopped], None, ones[~stopped], None, **kw)
    assert np.array_equal(gt_all, gt_live) and gt_all.any() and (gt_all <= 0).all()      # d log_T / d sigma = -step_ds < 0
    skip = GO.skip_distances(g["links"])
    a = DA.depth_backward(g, o, d, ones, ones, tape, **kw)
    b = DA.depth_backward(g, o, d, ones, ones, tape, skip=skip, **kw)
    assert np.array_equal(a, b)
    # hostile rays: nothing, whatever the cotangents hold
    ho = np.array([[0, 0, -3], [np.nan, 0, -3], [0, 0, -3], [np.inf, 0, 0], [0, 0, 30]], np.float32)
    hd = np.array([[0, 0, 0], [0, 0, 1], [np.inf, 0, 1], [0, 1, 0], [0, 0, 1]], np.float32)
    nan = np.full(5, np.nan, np.float32)
    dep, lt, tp = DA.depth_taped(g, ho, hd)
    assert not dep.any() and not lt.any() and not tp.any()
    assert not DA.depth_backward(g, ho, hd, nan, nan, tp).any()
    with pytest.raises(ValueError):
        DA.depth_backward(g, ho, hd, None, None, None)
    with pytest.raises(ValueError):
        DA.depth_backward(g, ho, hd, nan, None, None)
    assert DA.depth_backward(g, ho[:0], hd[:0], nan[:0], None, tp[:0]).shape == g["density_data"].shape


# ---- C ABI ------------------------------------------------------------------------------------------------------------
NEW_STRUCTS = {"nerf_grid_depth_taped_args": "GridDepthTapedArgs", "nerf_grid_depth_backward_args": "GridDepthBackwardArgs"}
NEW_SYMBOLS = ("nerf_grid_depth_rays_taped", "nerf_grid_depth_backward")


def test_depth_autograd_structs_match_a_c_compile_of_the_header(tmp_path):
    assert_structs_match_c_header(tmp_path, NEW_STRUCTS)


def test_depth_autograd_calls_refuse_bad_arguments_before_any_device_call():
    """Every refusal here comes before the handle is dereferenced or a kernel launched: the pointers are fakes."""
    import nerf_projects_amd  # noqa: F401
    from nerf_projects_amd import _lib
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in _lib.EXPORTS
    fake = C.c_void_p(0x1000)
    err = lambda: lib.nerf_last_error().decode()      # noqa: E731

    def options():
        opt = _lib.GridRenderOptions()
        opt.step_size, opt.sigma_thresh, opt.stop_thresh, opt.background_brightness = 0.5, 1e-10, 1e-7, 1.0
        return opt

    def taped(**kw):
        a = _lib.GridDepthTapedArgs()
        a.origins = a.dirs = a.depth = a.tape = 0x1000
        a.n_rays = 5
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def backward(**kw):
        a = _lib.GridDepthBackwardArgs()
        a.origins = a.dirs = a.grad_depth = a.grad_log_transmit = a.tape = a.grad_density = 0x1000
        a.n_rays = 5
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for fn, make, name in ((lib.nerf_grid_depth_rays_taped, taped, NEW_SYMBOLS[0]), (lib.nerf_grid_depth_backward, backward, NEW_SYMBOLS[1])):
        def refused(a, word, opt=None):
            assert fn(fake, C.byref(opt or options()), C.byref(a)) == -1 and word in err() and name in err(), (name, word, err())

        assert fn(None, C.byref(options()), C.byref(make())) == -1 and "NULL grid" in err()
        assert fn(fake, C.byref(options()), None) == -1 and "NULL" in err()
        assert fn(fake, None, C.byref(make())) == -1 and "NULL" in err()
        for delta in (-8, 8):
            a = make()
            a.struct_size += delta
            refused(a, "struct_size")
        opt = options()
        opt.struct_size += 4
        refused(make(), "struct_size", opt)
        for step in (0.0, -0.5, float("nan")):
            opt = options()
            opt.step_size = step
            refused(make(), "step_size", opt)
        for field in ("last_sample_opaque", "randomize"):
            opt = options()
            setattr(opt, field, 1)
            refused(make(), field, opt)
            assert "not built" in err()
        for kw in ({"n_rays": -1}, {"n_rays": (1 << 26) + 1}, {"origins": 0}, {"dirs": 0}):
            refused(make(**kw), "n_rays")
        assert fn(fake, C.byref(options()), C.byref(make(n_rays=0))) == 0      # zero rays: nothing is done
    # the taped forward's own
    for kw, word in (({"depth": 0}, "depth is NULL"), ({"tape": 0}, "tape is NULL")):
        assert lib.nerf_grid_depth_rays_taped(fake, C.byref(options()), C.byref(taped(**kw))) == -1 and word in err(), err()
    assert lib.nerf_grid_depth_rays_taped(fake, C.byref(options()), C.byref(taped(n_rays=0, depth=0, tape=0))) == 0
    # the backward's own
    for kw, word in (({"grad_depth": 0, "grad_log_transmit": 0, "tape": 0}, "both NULL"),
                     ({"grad_depth": 0, "grad_log_transmit": 0}, "both NULL"),
                     ({"grad_depth": 0}, "if and only if"),      # a tape without its cotangent
                     ({"tape": 0}, "if and only if"),            # a depth cotangent without the tape
                     ({"grad_density": 0}, "grad_density is NULL")):
        assert lib.nerf_grid_depth_backward(fake, C.byref(options()), C.byref(backward(**kw))) == -1 and word in err(), (kw, err())
        assert "nerf_grid_depth_backward" in err()
    assert lib.nerf_grid_depth_backward(fake, C.byref(options()), C.byref(backward(n_rays=0, grad_depth=0, grad_log_transmit=0))) == -1


def test_module_refusals_that_need_no_device():
    """ValueError for a bad threshold before the grid, the rays or a device are looked at (the module is assembled by hand,
    without a grid), and the argument checks of the rays."""
    import nerf_projects_amd as N
    from nerf_projects_amd import grid_autograd
    m = N.GridModule.__new__(N.GridModule)
    for bad in (-1.0, -1e-30, float("nan"), float("-inf")):
        with pytest.raises(ValueError, match="sigma_thresh"):
            m.volume_render_depth(None, sigma_thresh=bad)
        with pytest.raises(ValueError, match="sigma_thresh"):
            grid_autograd.GridModule.volume_render_depth_image(m, None, sigma_thresh=bad)
    with pytest.raises(ValueError, match="return_log_transmit"):
        m.volume_render_depth(None, sigma_thresh=1.0, return_log_transmit=True)
    with pytest.raises(NotImplementedError, match="use_kernel"):
        m.volume_render(None, use_kernel=False, return_log_transmit=True)
    with pytest.raises(TypeError, match="SparseGrid"):
        N.GridModule(object())
    with pytest.raises(RuntimeError, match="CPU"):
        grid_autograd._points_arg(torch.zeros(4, 3), "rays.origins", torch.device("cuda"))
    for name in ("volume_render_depth", "volume_render_depth_image"):
        assert callable(getattr(N.GridModule, name))
    doc = grid_autograd.__doc__
    assert "volume_render_depth" in doc and "of depth or" not in doc      # no longer listed as not built


def test_grid_depth_autograd_kernels_generated_code(tmp_path):
    """No scratch, no LDS, no inline assembly, no compare-and-swap: every float add is one hardware atomic without return.
    At most 64 VGPRs: 8 waves per SIMD, which is what hides the dependent skip -> link -> density loads. The device functions
    of the march are grid_device.h's, used and not copied."""
    text, asm, build = compile_kernels_to_asm(tmp_path, "grid_depth_autograd_kernels.hip")
    assert "grid_depth_autograd_kernels.hip" in build.SOURCES and "grid_depth_autograd_api.cpp" in build.SOURCES
    assert not re.search(r"\basm\b|__asm", text) and "__shared__" not in text
    for fn in ("setup_ray", "march_cell", "skip_jump", "load_links", "sample_sigma"):
        assert re.search(r"\b%s\b" % fn, text) and not re.search(r"\b(void|float|int)\s+%s\b" % fn, text), fn
    kernels = re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M)
    assert sum("grid_depth_taped_kernel" in k for k in kernels) == 2 and sum("grid_depth_bwd_kernel" in k for k in kernels) == 2
    assert len(kernels) == 4, kernels      # each with and without skip data
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)
    assert len(sizes) == len(kernels) and all(int(s) == 0 for s in sizes), sizes
    lds = re.findall(r"\.group_segment_fixed_size:\s*(\d+)", asm)
    assert len(lds) == len(kernels) and all(int(s) == 0 for s in lds), lds
    assert not re.search(r"\bscratch_(load|store)", asm)
    assert "cmpswap" not in asm
    assert len(re.findall(r"\bglobal_atomic_add_f32\b", asm)) == 16      # 8 corners in each of the two backward kernels
    assert not re.search(r"global_atomic_add_f32[^\n]*\bsc0\b", asm)      # none returns the old value
    vgprs = dict(zip(kernels, (int(v) for v in re.findall(r"\.vgpr_count:\s*(\d+)", asm))))
    print("vgprs per kernel:", vgprs)
    assert len(vgprs) == 4 and max(vgprs.values()) <= 64
