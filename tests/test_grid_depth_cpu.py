"""Sparse voxel grid depth and ray lengths, the parts that need no GPU: the numpy restatement (tests/grid_depth_oracle.py)
against what the reference's renderer gives (tests/golden/grid_depth.npz), against the colour march of tests/grid_oracle.py
and against a closed form, the C ABI of the new entry points, and the generated code of csrc/grid_depth_kernels.hip."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_depth_oracle as DO  # noqa: E402
import grid_oracle as GO  # noqa: E402
from grid_testlib import assert_structs_match_c_header, compile_kernels_to_asm  # noqa: E402
from test_grid_cpu import GRIDS, fixture_grid, load_fixture  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "grid_depth.npz")
THRESHOLDS = (0.0, 5.0, 40.0)


def load_depth_fixture():
    return np.load(FIXTURE)      # (allow_pickle is off: arrays only)


def grid_e(z):
    return {"links": z["e_links"], "density_data": z["e_density"], "sh_data": z["e_sh"], "radius": z["e_radius"],
            "center": z["e_center"]}


def raylen_cases(z, name):
    """(near_clip, recorded fp32 ray lengths) of a grid"""
    cases = [(0.0, z[f"{name}_raylen"])]
    if name == "a":
        cases.append((float(z["raylen_near"]), z["a_raylen_near"]))
    return cases


_march = {}


def marches(name):
    """The oracle's marches of a fixture grid at thresholds 0, computed once: ``{(skip, threshold): (depth, log_transmit)}``."""
    if name not in _march:
        zr = load_fixture()
        g = fixture_grid(zr, name)
        o, d = zr[f"{name}_origins"], zr[f"{name}_dirs"]
        skip = GO.skip_distances(g["links"])
        res = {}
        for sk in (None, skip):
            for x in (None,) + THRESHOLDS:
                res[(sk is not None, x)] = DO.depth(g, o, d, sigma_thresh=0.0, stop_thresh=0.0, skip=sk, threshold=x)
        _march[name] = res
    return _march[name]


def test_fixture_is_what_the_issue_asks_for():
    assert os.path.getsize(FIXTURE) < 1 << 20
    z = load_depth_fixture()
    zr = load_fixture()
    for name in GRIDS:
        for _, want in raylen_cases(z, name):
            assert want.dtype == np.float32 and want.shape == (len(zr[f"{name}_origins"]),)
            assert np.isfinite(want).all() and (want < 0).sum() >= 90 and (want > 0).sum() >= 800
        assert z[f"{name}_raylen64"].dtype == np.float64
    assert 0 < float(z["raylen_d_ref"]) < 1e-4
    links, dens, sh = z["e_links"], z["e_density"], z["e_sh"]
    assert links.shape == (12, 10, 14) and np.array_equal(links.reshape(-1), np.arange(links.size))      # every node kept
    assert sh.shape == (links.size, 3) and dens.shape == (links.size, 1)
    vol = dens.reshape(links.shape)
    assert vol.min() < -3 and vol.max() > 19
    inner = np.zeros(links.shape, dtype=bool)
    inner[1:-1, 1:-1, 1:-1] = True
    assert (vol[~inner] == 0).all() and (vol[inner] != 0).mean() > 0.9      # the outermost node layer is exactly empty
    i, j, k = np.meshgrid(*(np.arange(s) for s in links.shape), indexing="ij")
    pos = np.stack([i / 12, j / 10, k / 14], -1).reshape(-1, 3)
    assert np.abs(sh * GO.SH_C0 + 0.5 - pos).max() < 1e-6      # the colour of a node is its position
    assert (z["e_depth64"] > 0).mean() >= 0.8 and z["e_depth64"].max() > 3.0
    assert 0 < float(z["e_d_ref"]) < 1e-4


def test_oracle_gives_the_depth_of_the_references_renderer_on_grid_e():
    z = load_depth_fixture()
    g = grid_e(z)
    tol = 3.0 * float(z["e_d_ref"])
    skip = GO.skip_distances(g["links"])
    for sk in (None, skip):
        depth, log_t = DO.depth(g, z["e_origins"], z["e_dirs"], sigma_thresh=0.0, stop_thresh=0.0, skip=sk)
        assert depth.dtype == np.float32 and log_t.dtype == np.float32
        err = np.abs(depth.astype(np.float64) - z["e_depth64"])
        print(f"grid e: oracle vs the reference's renderer max {err.max():.3e} (bar {tol:.3e}), T max "
              f"{np.abs(np.exp(log_t.astype(np.float64)) - z['e_T64']).max():.3e}")
        assert err.max() <= tol, (int(err.argmax()), err.max())      # every ray
        assert np.abs(np.exp(log_t.astype(np.float64)) - z["e_T64"]).max() <= tol
    d64, _ = DO.depth(g, z["e_origins"], z["e_dirs"], sigma_thresh=0.0, stop_thresh=0.0, dtype=np.float64)
    assert d64.dtype == np.float64 and np.abs(d64 - z["e_depth64"]).max() <= tol


@pytest.mark.parametrize("name", GRIDS)
def test_oracle_walks_the_colour_march(name):
    """log_transmit is the colour oracle's bit for bit (which is pinned to the reference on these grids), with and without
    skip data; the depth does not change with skip data."""
    zr = load_fixture()
    g = fixture_grid(zr, name)
    o, d = zr[f"{name}_origins"], zr[f"{name}_dirs"]
    skip = GO.skip_distances(g["links"])
    res = marches(name)
    _, want = GO.render(g, o, d, sigma_thresh=0.0, stop_thresh=0.0)
    for sk in (False, True):
        assert np.array_equal(res[(sk, None)][1], want), (name, sk)
    assert np.array_equal(res[(False, None)][0], res[(True, None)][0])
    assert (res[(False, None)][1] < 0).sum() > 20
    # the default thresholds, near_clip and another step: the early stop at -1e3 included
    for kw in ({}, {"near_clip": 6.0, "step_size": 0.3}) if name == "a" else ({},):
        _, want = GO.render(g, o, d, **kw)
        plain = DO.depth(g, o, d, **kw)
        acc = DO.depth(g, o, d, skip=skip, **kw)
        assert np.array_equal(plain[1], want) and np.array_equal(acc[1], want), (name, kw)
        assert np.array_equal(plain[0], acc[0]), (name, kw)
        assert (want == np.float32(-1e3)).any() or name == "d"      # (one node of density 25 saturates no ray)
        for x in THRESHOLDS:      # the threshold mode with skip data, too
            assert np.array_equal(DO.depth(g, o, d, threshold=x, **kw)[0], DO.depth(g, o, d, threshold=x, skip=skip, **kw)[0])


@pytest.mark.parametrize("name", GRIDS)
def test_oracle_gives_the_references_ray_lengths(name):
    z = load_depth_fixture()
    zr = load_fixture()
    g = fixture_grid(zr, name)
    tol = 3.0 * float(z["raylen_d_ref"])
    for near, want in raylen_cases(z, name):
        got = DO.ray_lengths(g, zr[f"{name}_origins"], zr[f"{name}_dirs"], near_clip=near)
        fin = np.isfinite(want)
        err = np.abs(got[fin].astype(np.float64) - want[fin])
        print(f"grid {name} near_clip {near}: ray lengths vs reference max {err.max():.3e} (bar {tol:.3e})")
        assert got.dtype == np.float32 and np.array_equal(np.isfinite(got), fin) and err.max() <= tol
        assert np.array_equal(np.sign(got[fin]), np.sign(want[fin]))      # the same rays miss
    # a set-up that is not finite: NaN
    o = np.array([[0, 0, -3], [np.nan, 0, -3], [0, 0, -3], [np.inf, 0, 0], [0, 0, -3]], np.float32)
    d = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 0], [0, 1, 0], [np.inf, 0, 1]], np.float32)
    got = DO.ray_lengths(g, o, d)
    assert np.isfinite(got[0]) and np.isnan(got[1:]).all()
    dep, lt = DO.depth(g, o, d)
    assert (dep[1:] == 0).all() and (lt[1:] == 0).all()


def test_constant_density_is_a_geometric_series():
    """An independent closed form. In a dense 8^3 grid of density 3 everywhere (outer layer included: a clamped position
    interpolates it too) every sample between entry and exit has sigma = 3, so with q = exp(-step * 3 * delta_scale) and
    samples t_k = tmin + k step, k < K = floor((tmax - tmin) / step) + 1:
    depth = delta_scale * (tmin (1 - q^K) + step (1 - q) sum_k k q^k), and the threshold depth at 0 is tmin * delta_scale.
    Entry and exit come from an fp64 ray-box intersection here. Fewer than 30 samples, a handful of fp32 roundings each:
    relative 1e-5. Rays whose last sample lies within 1e-3 steps of the exit are left out: there fp32 and fp64 may
    disagree on K, which is no error of the march."""
    rng = np.random.default_rng(5)
    reso, radius, center = 8, np.array([1.0, 0.9, 1.1], np.float32), np.array([0.1, 0.0, -0.2], np.float32)
    n = reso ** 3
    g = {"links": np.arange(n, dtype=np.int32).reshape(reso, reso, reso), "density_data": np.full((n, 1), 3.0, np.float32),
         "sh_data": np.zeros((n, 3), np.float32), "radius": radius, "center": center}
    u = rng.normal(size=(512, 3))
    o = (center + 3.0 * radius * u / np.linalg.norm(u, axis=-1, keepdims=True)).astype(np.float32)
    d = ((center + radius * rng.uniform(-0.9, 0.9, (512, 3)) - o) * rng.uniform(0.2, 5.0, (512, 1))).astype(np.float32)
    step = 0.5
    r64, c64 = radius.astype(np.float64), center.astype(np.float64)
    og = (0.5 * (1.0 - c64 / r64) * reso - 0.5) + o.astype(np.float64) * (0.5 / r64 * reso)
    dg = d.astype(np.float64) / np.linalg.norm(d.astype(np.float64), axis=-1, keepdims=True) * (0.5 / r64 * reso)
    ds = 1.0 / np.linalg.norm(dg, axis=-1)
    dg *= ds[:, None]
    t1, t2 = (-0.5 - og) / dg, (reso - 0.5 - og) / dg
    tmin, tmax = np.maximum(np.minimum(t1, t2).max(-1), 0.0), np.maximum(t1, t2).min(-1)
    steps = (tmax - tmin) / step
    use = (tmax > tmin) & (np.abs(steps - np.round(steps)) > 1e-3)
    assert use.sum() > 400
    K = np.floor(steps) + 1
    assert K[use].max() < 30 and K[use].min() >= 1 and tmin[use].min() > 1.0
    q = np.exp(-step * 3.0 * ds)
    ksum = q * (1 - K * q ** (K - 1) + (K - 1) * q ** K) / (1 - q) ** 2
    want = ds * (tmin * (1 - q ** K) + step * (1 - q) * ksum)
    skip = GO.skip_distances(g["links"])
    assert skip.max() == 0
    for sk in (None, skip):
        got, log_t = DO.depth(g, o, d, step_size=step, sigma_thresh=0.0, stop_thresh=0.0, skip=sk)
        rel = np.abs(got[use] - want[use]) / want[use]
        print(f"geometric series: expected depth relative max {rel.max():.3e}, log_transmit "
              f"{np.abs(log_t[use] - K[use] * np.log(q[use])).max():.3e}")
        assert rel.max() <= 1e-5
        first, _ = DO.depth(g, o, d, step_size=step, threshold=0.0, skip=sk)
        assert (np.abs(first[use] - tmin[use] * ds[use]) / (tmin[use] * ds[use])).max() <= 1e-5
        # (interpolating the constant rounds: sigma is 3 up to an ulp, so the thresholds stay clear of 3)
        assert np.array_equal(DO.depth(g, o, d, step_size=step, threshold=2.5, skip=sk)[0], first)
        assert (DO.depth(g, o, d, step_size=step, threshold=3.5, skip=sk)[0] == 0).all()


@pytest.mark.parametrize("name", GRIDS)
def test_threshold_mode_properties(name):
    """At thresholds 0 a ray has a first sample with sigma > 0 exactly when its transmittance fell: depth > 0 exactly where
    log_transmit < 0 - on the rays that enter the box at t > 0; a ray that starts inside it (tmin = 0) may be hit at its very
    first sample, at distance 0, which only the implication covers. Where a higher threshold is still exceeded, it is
    exceeded no earlier."""
    zr = load_fixture()
    g = fixture_grid(zr, name)
    res = marches(name)
    _, _, _, _, tmin, _, _ = GO.ray_setup(g, zr[f"{name}_origins"], zr[f"{name}_dirs"])
    log_t = res[(False, None)][1]
    first = [res[(False, x)][0] for x in THRESHOLDS]
    outside = tmin > 0
    assert outside.sum() > 800
    assert np.array_equal(first[0][outside] > 0, log_t[outside] < 0)
    assert (log_t[first[0] > 0] < 0).all() and (first[0] >= 0).all()
    assert (first[0] > 0).sum() > 20
    for lo, hi in zip(first[:-1], first[1:]):
        hit = hi > 0
        assert (hi[hit] >= lo[hit]).all() and (lo[hit & outside] > 0).all()
    assert (first[1] > first[0]).any() or name == "d"      # (d holds one node of density 25)
    for x in THRESHOLDS:
        assert np.array_equal(res[(True, x)][0], res[(False, x)][0])      # skip data changes nothing
        assert (res[(False, x)][1] == 0).all()
    for bad in (-1.0, -1e-30, float("nan")):
        with pytest.raises(ValueError):
            DO.depth(g, zr[f"{name}_origins"][:2], zr[f"{name}_dirs"][:2], threshold=bad)


# ---- C ABI ------------------------------------------------------------------------------------------------------------
def test_depth_struct_matches_a_c_compile_of_the_header(tmp_path):
    from nerf_projects_amd import _lib
    modes = assert_structs_match_c_header(tmp_path, {"nerf_grid_depth_args": "GridDepthArgs"}, extra_prints=[
        'printf("mode expected %d\\n", NERF_GRID_DEPTH_EXPECTED);', 'printf("mode threshold %d\\n", NERF_GRID_DEPTH_THRESHOLD);',
        'printf("mode raylen %d\\n", NERF_GRID_DEPTH_RAYLEN);'])
    assert modes == {"mode": {"expected": _lib.NERF_GRID_DEPTH_EXPECTED, "threshold": _lib.NERF_GRID_DEPTH_THRESHOLD,
                              "raylen": _lib.NERF_GRID_DEPTH_RAYLEN}}
    assert sorted(modes["mode"].values()) == [0, 1, 2]


def test_depth_calls_refuse_bad_arguments_before_any_device_call():
    """Every refusal here comes before the handle is dereferenced or a kernel launched: the pointers are fakes."""
    import nerf_projects_amd  # noqa: F401
    from nerf_projects_amd import _lib
    lib = _lib.load()
    for s in ("nerf_grid_depth_rays", "nerf_grid_depth_image"):
        assert hasattr(lib, s) and s in _lib.EXPORTS
    fake = C.c_void_p(0x1000)
    err = lambda: lib.nerf_last_error().decode()      # noqa: E731
    opt = _lib.GridRenderOptions()
    opt.step_size, opt.sigma_thresh, opt.stop_thresh, opt.background_brightness = 0.5, 1e-10, 1e-7, 1.0
    cam = _lib.GridCamera()
    cam.fx = cam.fy = 30.0
    cam.width, cam.height = 4, 3

    def args(**kw):
        a = _lib.GridDepthArgs()
        a.origins = a.dirs = a.depth = 0x1000
        a.n_rays = 5
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def both(a, word):
        assert lib.nerf_grid_depth_rays(fake, C.byref(opt), C.byref(a)) == -1 and word in err(), err()
        assert "nerf_grid_depth_rays" in err()
        assert lib.nerf_grid_depth_image(fake, C.byref(cam), C.byref(opt), C.byref(a)) == -1 and word in err(), err()
        assert "nerf_grid_depth_image" in err()

    assert lib.nerf_grid_depth_rays(None, C.byref(opt), C.byref(args())) == -1 and "NULL grid" in err()
    assert lib.nerf_grid_depth_image(None, C.byref(cam), C.byref(opt), C.byref(args())) == -1 and "NULL grid" in err()
    assert lib.nerf_grid_depth_rays(fake, C.byref(opt), None) == -1 and "NULL" in err()
    assert lib.nerf_grid_depth_rays(fake, None, C.byref(args())) == -1 and "NULL" in err()
    assert lib.nerf_grid_depth_image(fake, None, C.byref(opt), C.byref(args())) == -1 and "nerf_grid_camera is NULL" in err()
    a = args()
    a.struct_size -= 8
    both(a, "struct_size")
    a = args()
    a.struct_size += 8
    both(a, "struct_size")
    for bad in (3, -1, 255):
        both(args(mode=bad), f"mode = {bad}")
    for bad in (-1.0, -1e-30, float("nan"), float("-inf")):
        both(args(mode=_lib.NERF_GRID_DEPTH_THRESHOLD, sigma_thresh=bad), "sigma_thresh")
    both(args(depth=0), "depth is NULL")
    for mode in (_lib.NERF_GRID_DEPTH_THRESHOLD, _lib.NERF_GRID_DEPTH_RAYLEN):
        both(args(mode=mode, log_transmit=0x1000), "log_transmit")
    for kw, word in (({"n_rays": -1}, "n_rays"), ({"n_rays": (1 << 26) + 1}, "n_rays"), ({"origins": 0}, "origins"),
                     ({"dirs": 0}, "origins and dirs")):
        assert lib.nerf_grid_depth_rays(fake, C.byref(opt), C.byref(args(**kw))) == -1 and word in err(), err()
    big = _lib.GridCamera()
    big.fx = big.fy = 30.0
    big.width, big.height = 1 << 14, (1 << 12) + 1
    assert lib.nerf_grid_depth_image(fake, C.byref(big), C.byref(opt), C.byref(args())) == -1 and "2^26" in err()
    opt.step_size = 0.0      # the render's option checks apply
    both(args(), "step_size")
    opt.step_size = 0.5
    opt.randomize = 1
    both(args(), "randomize")


def test_python_refuses_a_bad_threshold_before_anything_else():
    """ValueError before the grid, the rays or a device are looked at: the object is assembled by hand, without a handle."""
    import nerf_projects_amd  # noqa: F401
    from nerf_projects_amd.grid import RenderOptions, SparseGrid
    g = SparseGrid.__new__(SparseGrid)
    g.opt = RenderOptions()
    for bad in (-1.0, -1e-30, float("nan"), float("-inf")):
        with pytest.raises(ValueError, match="sigma_thresh"):
            g.volume_render_depth(None, sigma_thresh=bad)
        with pytest.raises(ValueError, match="sigma_thresh"):
            g.volume_render_depth_image(None, sigma_thresh=bad)
    with pytest.raises(ValueError, match="return_log_transmit"):
        g.volume_render_depth(None, sigma_thresh=1.0, return_log_transmit=True)
    with pytest.raises(NotImplementedError, match="use_kernel"):
        g.volume_render(None, use_kernel=False, return_raylen=True)
    with pytest.raises(NotImplementedError, match="randomize"):
        g.volume_render(None, randomize=True, return_raylen=True)


def test_grid_depth_kernels_generated_code(tmp_path):
    """One lane per ray and nothing shared: no scratch, no LDS, no atomics, no inline assembly, no cross-lane operation. At
    most 64 VGPRs: 8 waves per SIMD, which is what hides the dependent skip -> link -> density loads."""
    text, asm, build = compile_kernels_to_asm(tmp_path, "grid_depth_kernels.hip")
    assert "grid_depth_kernels.hip" in build.SOURCES and "grid_depth_api.cpp" in build.SOURCES
    assert not re.search(r"\basm\b|__asm", text)
    assert not re.search(r"atomic\w*\(", text) and "__shared__" not in text and "__shfl" not in text
    for fn in ("setup_ray", "march_cell", "skip_jump", "load_links", "sample_sigma", "camera_ray"):
        assert re.search(r"\b%s\b" % fn, text) and not re.search(r"\b(void|float|int)\s+%s\b" % fn, text), fn      # used, not copied
    kernels = re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M)
    assert len(kernels) == 10 and all("grid_depth_kernel" in k for k in kernels), kernels      # 2 marches x rays/image x skip, 2 lengths
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)
    assert len(sizes) == len(kernels) and all(int(s) == 0 for s in sizes), sizes
    lds = re.findall(r"\.group_segment_fixed_size:\s*(\d+)", asm)
    assert len(lds) == len(kernels) and all(int(s) == 0 for s in lds), lds
    assert not re.search(r"\bscratch_(load|store)", asm)
    assert not re.search(r"^\s*(global|flat|buffer|ds)_atomic", asm, re.M)
    assert not re.search(r"^\s*ds_", asm, re.M) and "v_readlane" not in asm and "dpp" not in asm
    vgprs = [int(v) for v in re.findall(r"\.vgpr_count:\s*(\d+)", asm)]
    print("vgprs per kernel:", dict(zip(kernels, vgprs)))
    assert len(vgprs) == len(kernels) and max(vgprs) <= 64
