"""Sparse voxel grid training, the parts that need no GPU: the numpy restatement (tests/grid_train_oracle.py) against the
reference's recorded gradients (also off the recorded setting: tests/golden/grid_train_variants.npz) and its recorded RMSProp
loop, its total-variation gradient against an fp64 autograd statement, the C ABI of the training entry points, and the
generated code of csrc/grid_train_kernels.hip."""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_oracle as GO  # noqa: E402
import grid_train_oracle as GT  # noqa: E402
from grid_testlib import assert_structs_match_c_header, compile_kernels_to_asm  # noqa: E402

RENDER = os.path.join(ROOT, "tests", "golden", "grid_render.npz")
TRAIN = os.path.join(ROOT, "tests", "golden", "grid_train.npz")
VARIANTS = os.path.join(ROOT, "tests", "golden", "grid_train_variants.npz")
GRIDS = ("a", "b", "c", "d")
VARIANT_CASES = (("a", "step"), ("a", "near"), ("a", "mix"), ("b", "mix"), ("c", "mix"))


def fixture_grid(z, name):
    return {"links": z[f"{name}_links"], "density_data": z[f"{name}_density"], "sh_data": z[f"{name}_sh"],
            "radius": z[f"{name}_radius"], "center": z[f"{name}_center"]}


def grad_bar(t, name, tag, key):
    """3x the reference's own fp32 - fp64 distance, and no tighter than 1e-5 of the tensor's largest entry"""
    want = t[f"{name}_{tag}_grad_{key}64"].astype(np.float64)
    return want, max(3.0 * float(t[f"{name}_{tag}_grad_{key}_d_ref"]), 1e-5 * float(np.abs(want).max()))


@functools.lru_cache(maxsize=None)
def variant_oracle(name, tag):
    """(rgb, grad_density, grad_sh, mask) of the restatement at a setting of grid_train_variants.npz; computed once and
    shared by the CPU and the GPU test (read only)"""
    z, t, v = np.load(RENDER), np.load(TRAIN), np.load(VARIANTS)
    bg, step, near = v[f"{name}_{tag}_variant"].tolist()
    out = GT.fused(fixture_grid(z, name), z[f"{name}_origins"], z[f"{name}_dirs"], t[f"{name}_rgb_gt"], step_size=step,
                   sigma_thresh=0.0, stop_thresh=0.0, background_brightness=bg, near_clip=near)
    for a in out:
        a.setflags(write=False)
    return out


def test_fixture_holds_arrays_only_and_is_small():
    assert os.path.getsize(TRAIN) < 1 << 20
    t = np.load(TRAIN)      # (allow_pickle is off: arrays only)
    for name in GRIDS:
        assert t[f"{name}_rgb_gt"].shape == (1024, 3)
        for tag in ("bg1", "bg0"):
            assert t[f"{name}_{tag}_grad_density64"].shape[1] == 1
    for name in ("b", "c"):
        assert t[f"{name}_loop_idx"].shape == (20, 256) and t[f"{name}_loop_idx"].max() < 704
        assert t[f"{name}_loop_params"].tolist() == [0.95, 1e-8, 1e-2, 1.0]
        l32, l64 = t[f"{name}_loop_loss32"], t[f"{name}_loop_loss64"]
        assert np.abs(l32 - l64).max() < 1e-3 * (l64[0] - l64[-1])      # a test of the optimisation, not of noise


@pytest.mark.parametrize("name", GRIDS)
def test_oracle_gradients_match_the_reference_autograd(name):
    z, t = np.load(RENDER), np.load(TRAIN)
    g = fixture_grid(z, name)
    o, d, gt = z[f"{name}_origins"], z[f"{name}_dirs"], t[f"{name}_rgb_gt"]
    skip = GO.skip_distances(g["links"])
    for tag, bg in (("bg1", 1.0), ("bg0", 0.0)):
        rgb, gd, gs, mask = GT.fused(g, o, d, gt, sigma_thresh=0.0, stop_thresh=0.0, background_brightness=bg)
        fwd, _ = GO.render(g, o, d, sigma_thresh=0.0, stop_thresh=0.0, background_brightness=bg)
        assert np.array_equal(rgb, fwd)      # the restatement walks the renderer's lattice
        touched = np.zeros(mask.shape, dtype=bool)
        for key, got in (("density", gd), ("sh", gs)):
            want, tol = grad_bar(t, name, tag, key)
            err = np.abs(got.astype(np.float64) - want)
            print(f"grid {name} {tag} d/d{key}: oracle vs fp64 autograd max {err.max():.3e} (bar {tol:.3e}, max |g| {np.abs(want).max():.3e})")
            assert err.max() <= tol, (name, tag, key, int(err.argmax()), err.max(), tol)      # every entry
            touched |= (want != 0).any(-1)
        assert np.array_equal(mask != 0, touched), (name, tag, int((mask != 0).sum()), int(touched.sum()))
        # skip data changes no sample: the same colours and rows; the terms of a row's sum arrive in another order (rays
        # that jump fall into other passes of the vectorised loop), so the sums agree to their fp32 rounding
        rgb_s, gd_s, gs_s, mask_s = GT.fused(g, o, d, gt, sigma_thresh=0.0, stop_thresh=0.0, background_brightness=bg, skip=skip)
        assert np.array_equal(rgb_s, rgb) and np.array_equal(mask_s, mask)
        assert np.abs(gd_s - gd).max() <= 1e-5 * np.abs(gd).max() and np.abs(gs_s - gs).max() <= 1e-5 * np.abs(gs).max()
    # gradients accumulate
    _, gd2, gs2, _ = GT.fused(g, o, d, gt, sigma_thresh=0.0, stop_thresh=0.0, background_brightness=0.0, grad_density=gd.copy(),
                              grad_sh=gs.copy(), mask=mask.copy())
    assert np.abs(gd2 - 2 * gd).max() <= 1e-5 * np.abs(gd).max() and np.abs(gs2 - 2 * gs).max() <= 1e-5 * np.abs(gs).max()


def test_variants_fixture_holds_arrays_only_and_is_small():
    assert os.path.getsize(VARIANTS) < 1 << 20
    v = np.load(VARIANTS)      # (allow_pickle is off: arrays only)
    z = np.load(RENDER)
    assert VARIANT_CASES == (("a", "step"), ("a", "near"), ("a", "mix"), ("b", "mix"), ("c", "mix"))
    want = {"step": [1.0, 0.3, 0.0], "near": [1.0, 0.5, 6.0], "mix": [0.5, 0.8, 2.5]}
    for name, tag in VARIANT_CASES:
        assert v[f"{name}_{tag}_variant"].tolist() == want[tag]
        assert v[f"{name}_{tag}_grad_density64"].shape == z[f"{name}_density"].shape
        assert v[f"{name}_{tag}_grad_sh64"].shape == z[f"{name}_sh"].shape
        assert v[f"{name}_{tag}_grad_density64"].dtype == np.float32 and v[f"{name}_{tag}_loss64"].dtype == np.float64


@pytest.mark.parametrize("name,tag", VARIANT_CASES)
def test_oracle_gradients_match_the_reference_autograd_off_the_recorded_setting(name, tag):
    """step_size * delta_scale, the background's part of `remaining` and the clamp of tmin to near_clip are constant or
    vanish at the setting of grid_train.npz; here they do not. Measured, restatement vs fp64 autograd as a part of the largest
    entry (density, sh): a step 3.4e-5, 2.5e-5; a near 1.2e-4, 8.8e-6; a mix 2.0e-5, 9.2e-6; b mix 7.6e-6, 9.7e-6; c mix
    5.1e-6, 1.3e-6; all but one are within a few per cent of the reference's own fp32 - fp64 distance d_ref."""
    z, t, v = np.load(RENDER), np.load(TRAIN), np.load(VARIANTS)
    g = fixture_grid(z, name)
    bg, step, near = v[f"{name}_{tag}_variant"].tolist()
    rgb, gd, gs, mask = variant_oracle(name, tag)
    fwd, _ = GO.render(g, z[f"{name}_origins"], z[f"{name}_dirs"], step_size=step, sigma_thresh=0.0, stop_thresh=0.0,
                       background_brightness=bg, near_clip=near)
    assert np.array_equal(rgb, fwd)
    loss = float(((rgb.astype(np.float64) - t[f"{name}_rgb_gt"]) ** 2).mean())
    assert abs(loss - float(v[f"{name}_{tag}_loss64"])) <= 1e-5
    touched = np.zeros(mask.shape, dtype=bool)
    for key, got in (("density", gd), ("sh", gs)):
        want, tol = grad_bar(v, name, tag, key)
        err = np.abs(got.astype(np.float64) - want)
        print(f"grid {name} {tag} d/d{key}: oracle vs fp64 autograd max {err.max():.3e} = {err.max() / np.abs(want).max():.2e} of the "
              f"largest entry (bar {tol:.3e}, d_ref {float(v[f'{name}_{tag}_grad_{key}_d_ref']):.3e})")
        assert err.max() <= tol, (name, tag, key, int(err.argmax()), err.max(), tol)      # every entry
        touched |= (want != 0).any(-1)
    assert 0 < touched.sum() and np.array_equal(mask != 0, touched), (name, tag, int((mask != 0).sum()), int(touched.sum()))
    for key in ("density", "sh"):      # the variant is not the recorded setting in disguise: its gradients are far from bg1's
        base, tol = grad_bar(t, name, "bg1", key)
        assert np.abs(grad_bar(v, name, tag, key)[0] - base).max() > 100 * tol


def numpy_loop(z, t, name):
    """the 20 iterations of the fixture through the restatement: losses, final tables, per-iteration masks"""
    g = fixture_grid(z, name)
    g["density_data"] = (np.float32(0.5) * g["density_data"]).astype(np.float32)
    g["sh_data"] = np.zeros_like(g["sh_data"])
    beta, eps, lr_sh, lr_sigma = t[f"{name}_loop_params"].tolist()
    o, d = z[f"{name}_origins"][:704], z[f"{name}_dirs"][:704]
    target = z[f"{name}_bg1_rgb64"][:704].astype(np.float32)
    rms_d, rms_s = np.zeros_like(g["density_data"]), np.zeros_like(g["sh_data"])
    losses, masks = [], []
    for k in t[f"{name}_loop_idx"]:
        rgb, gd, gs, mask = GT.fused(g, o[k], d[k], target[k], sigma_thresh=0.0, stop_thresh=0.0)
        losses.append(float(((rgb.astype(np.float64) - target[k]) ** 2).mean()))
        GT.optim_step(g["density_data"], rms_d, gd, mask, "rmsprop", lr_sigma, beta, eps)
        GT.optim_step(g["sh_data"], rms_s, gs, mask, "rmsprop", lr_sh, beta, eps)
        masks.append(mask != 0)
    return np.array(losses), g["density_data"], g["sh_data"], np.stack(masks)


def loop_bars(t, name):
    l32, l64 = t[f"{name}_loop_loss32"], t[f"{name}_loop_loss64"]
    bars = {"loss": max(3.0 * float(np.abs(l32 - l64).max()), 1e-5 * float(l64[0]))}
    for key in ("density", "sh"):
        a32, a64 = t[f"{name}_loop_{key}32"].astype(np.float64), t[f"{name}_loop_{key}64"]
        bars[key] = max(3.0 * float(np.abs(a32 - a64).max()), 1e-5 * float(np.abs(a64).max()))
    return bars


@pytest.mark.parametrize("name", ("b", "c"))
def test_oracle_loop_matches_the_reference_loop(name):
    z, t = np.load(RENDER), np.load(TRAIN)
    losses, dens, sh, masks = numpy_loop(z, t, name)
    bars = loop_bars(t, name)
    l64 = t[f"{name}_loop_loss64"]
    print(f"grid {name}: loss {losses[0]:.5f} -> {losses[-1]:.5f}; vs fp64 max {np.abs(losses - l64).max():.2e} (bar {bars['loss']:.2e}); "
          f"density {np.abs(dens - t[name + '_loop_density64']).max():.2e} (bar {bars['density']:.2e}); "
          f"sh {np.abs(sh - t[name + '_loop_sh64']).max():.2e} (bar {bars['sh']:.2e})")
    assert losses[-1] < 0.7 * losses[0]
    assert np.abs(losses - l64).max() <= bars["loss"]
    assert np.abs(dens - t[f"{name}_loop_density64"]).max() <= bars["density"]
    assert np.abs(sh - t[f"{name}_loop_sh64"]).max() <= bars["sh"]
    want = np.unpackbits(t[f"{name}_loop_mask64"], axis=-1)[:, :masks.shape[1]].astype(bool)
    assert np.array_equal(masks, want)      # the touched rows of every iteration


def test_oracle_optimiser_and_tv_basics():
    rng = np.random.default_rng(3)
    data = rng.normal(size=(6, 4)).astype(np.float32)
    rms = np.zeros_like(data)
    rms[1] = 0.25
    grad = rng.normal(size=(6, 4)).astype(np.float32)
    mask = np.array([1, 1, 0, 0, 1, 0], dtype=np.uint8)
    d0, r0 = data.copy(), rms.copy()
    GT.optim_step(data, rms, grad, mask, "rmsprop", 0.1)
    assert np.array_equal(data[mask == 0], d0[mask == 0]) and np.array_equal(rms[mask == 0], r0[mask == 0])
    assert np.array_equal(rms[0], grad[0] * grad[0])      # first touch: rms = g^2, the step is lr * sign(g) up to eps
    assert np.allclose(data[0], d0[0] - 0.1 * np.sign(grad[0]), atol=1e-6)
    assert np.allclose(rms[1], grad[1] ** 2 + 0.95 * (0.25 - grad[1] ** 2), rtol=1e-6)
    # TV: a constant field over fully kept nodes adds nothing; the four adds of a cell sum to rounding
    links = np.arange(4 * 5 * 6, dtype=np.int32).reshape(4, 5, 6)
    g = {"links": links, "density_data": np.full((120, 1), 3.0, np.float32), "sh_data": rng.normal(size=(120, 3)).astype(np.float32),
         "radius": np.ones(3, np.float32), "center": np.zeros(3, np.float32)}
    grad_d, m = np.zeros((120, 1), np.float32), np.zeros(120, np.uint8)
    interior = links[1, 1, 1]
    GT.tv_grad(g, "density", int(interior), 3, 0.5, grad_d, m)
    assert not grad_d.any() and not m.any()
    grad_s = np.zeros((120, 3), np.float32)
    GT.tv_grad(g, "sh", int(interior), 1, 0.5, grad_s, m)
    assert m.sum() == 4 and np.abs(grad_s.sum(0)).max() <= 1e-6 * np.abs(grad_s).max()
    grad_w = np.zeros((120, 3), np.float32)
    GT.tv_grad(g, "sh", 118, 5, 0.5, grad_w, m)      # wraps past the last node
    assert grad_w[118].any() and grad_w[119].any() and grad_w[0].any() and grad_w[2].any() and not grad_w[40].any()


# ---- total variation against an independent statement ---------------------------------------------------------------
TV_LATTICES = ((12, 12, 12), (9, 12, 7), (2, 6, 5))
# (target, start_dim, end_dim): both tables and a column sub-range
TV_TARGETS = (("density", 0, None), ("sh", 0, None), ("sh", 3, 7))
TV_SCALING = 0.7


def tv_lattice(reso):
    """A grid (basis_dim 4) for the TV tests: nodes kept at random over the whole lattice with every face, edge and corner
    populated, links < -1, and a plateau: a block of kept nodes whose values are all equal, so that the nodes inside it
    receive only zeros. Returns (grid, rows inside the plateau)."""
    rng = np.random.default_rng(sum(reso))
    kept = rng.random(reso) < 0.6
    kept[::reso[0] - 1, ::reso[1] - 1, ::reso[2] - 1] = True
    block = tuple(slice(0, 2) if s == 2 else slice(1, 5) for s in reso)
    inside = tuple(slice(0, 1) if s == 2 else slice(2, 4) for s in reso)      # both neighbours along every axis are in the block
    kept[block] = True
    n = int(kept.sum())
    links = np.full(reso, -1, dtype=np.int32)
    links[kept] = rng.permutation(n).astype(np.int32)
    low = (~kept) & (rng.random(reso) < 0.3)
    links[low] = rng.integers(-9, -1, int(low.sum())).astype(np.int32)
    dens = rng.uniform(-2.0, 30.0, (n, 1)).astype(np.float32)
    sh = rng.normal(0.0, 0.7, (n, 12)).astype(np.float32)
    dens[links[block].ravel()] = 1.5
    sh[links[block].ravel()] = -0.25
    g = {"links": links, "density_data": dens, "sh_data": sh, "radius": np.ones(3, np.float32), "center": np.zeros(3, np.float32)}
    for face in (links[0], links[-1], links[:, 0], links[:, -1], links[:, :, 0], links[:, :, -1]):
        assert (face >= 0).any()
    return g, links[inside].ravel()


def tv_grad_fp64(links, table, scale, start_dim=0, end_dim=None):
    """The TV gradient over ALL nodes, stated independently of the kernel and of tests/grid_train_oracle.py: fp64 autograd.
    v = the lattice of table values, 0 at empty (any link outside [0, capacity)) nodes and beyond the upper faces; dx, dy, dz
    forward differences; inv = scale / sqrt(1e-9 + dx^2 + dy^2 + dz^2), held constant; the gradient of
    sum(0.5 inv (s_x dx^2 + s_y dy^2 + s_z dz^2)) with s = size / 256 (fp32). On a cubic lattice that is the gradient of
    s * scale * sum(sqrt(1e-9 + |forward differences|^2)), the TV loss itself."""
    import torch
    cap = table.shape[0]
    t = torch.tensor(table.astype(np.float64), requires_grad=True)
    lk = torch.from_numpy(links.astype(np.int64))
    present = (lk >= 0) & (lk < cap)
    v = torch.where(present[..., None], t[lk.clamp(0, cap - 1)][..., start_dim:end_dim], torch.zeros((), dtype=torch.float64))
    vp = torch.nn.functional.pad(v, (0, 0, 0, 1, 0, 1, 0, 1))      # zeros beyond the upper faces
    dx, dy, dz = vp[1:, :-1, :-1] - v, vp[:-1, 1:, :-1] - v, vp[:-1, :-1, 1:] - v
    inv = (float(scale) / torch.sqrt(1e-9 + dx * dx + dy * dy + dz * dz)).detach()
    sx, sy, sz = (float(np.float32(s) * np.float32(1.0 / 256.0)) for s in links.shape)
    (0.5 * inv * (sx * dx * dx + sy * dy * dy + sz * dz * dz)).sum().backward()
    return t.grad.numpy()


@functools.lru_cache(maxsize=None)
def tv_case(reso, target, start_dim, end_dim):
    """(grid, plateau rows, scale, fp64 gradient, restated gradient, restated mask) with every node covered by a range that
    wraps: start = n - 1, count = n. Computed once, shared by the CPU and the GPU test (read only)."""
    g, plateau = tv_lattice(reso)
    n = g["links"].size
    table = g["density_data"] if target == "density" else g["sh_data"]
    scale = np.float32(TV_SCALING / n)
    want64 = tv_grad_fp64(g["links"], table, scale, start_dim, end_dim)
    grad, mask = np.zeros_like(table), np.zeros(table.shape[0], np.uint8)
    GT.tv_grad(g, target, n - 1, n, scale, grad, mask, start_dim, end_dim)
    for a in (want64, grad, mask):
        a.setflags(write=False)
    return g, plateau, scale, want64, grad, mask


@pytest.mark.parametrize("target,start_dim,end_dim", TV_TARGETS)
@pytest.mark.parametrize("reso", TV_LATTICES)
def test_oracle_tv_gradient_matches_the_fp64_autograd_statement(reso, target, start_dim, end_dim):
    """The bar, 1e-5 of the largest entry: an entry is the sum of at most 6 terms of about 6 fp32 roundings each, 36 * 6e-8 =
    2e-6 of the largest term. Measured: at most 1.9e-7 of the largest entry over the nine cases."""
    g, plateau, scale, want64, grad, mask = tv_case(reso, target, start_dim, end_dim)
    big = float(np.abs(want64).max())
    err = float(np.abs(grad.astype(np.float64) - want64).max())
    print(f"tv {reso} {target}[{start_dim}:{end_dim}]: restatement vs fp64 autograd max {err:.3e} = {err / big:.2e} of the largest entry")
    assert big > 0 and err <= 1e-5 * big
    # the mask is exactly the rows that receive a non-zero value: none inside the plateau, every other kept row here
    sl = slice(start_dim, end_dim)
    assert np.array_equal(mask != 0, (want64[:, sl] != 0).any(-1))
    assert len(plateau) and not mask[plateau].any() and not grad[plateau].any()
    assert mask.sum() >= mask.size - 4 * len(plateau)
    out = np.ones(grad.shape[1], bool)
    out[sl] = False
    assert not grad[:, out].any() and not want64[:, out].any()


# ---- C ABI ------------------------------------------------------------------------------------------------------------
NEW_STRUCTS = {"nerf_grid_fused_args": "GridFusedArgs", "nerf_grid_tv_args": "GridTvArgs", "nerf_grid_optim_args": "GridOptimArgs"}
NEW_SYMBOLS = ("nerf_grid_fused_backward", "nerf_grid_tv_grad", "nerf_grid_optim_step")


def test_training_structs_match_a_c_compile_of_the_header(tmp_path):
    import nerf_projects_amd  # noqa: F401
    from nerf_projects_amd import _lib
    consts = assert_structs_match_c_header(tmp_path, NEW_STRUCTS, extra_prints=[
        'printf("consts tv %d\\n", NERF_GRID_TV_DENSITY * 10 + NERF_GRID_TV_SH);',
        'printf("consts optim %d\\n", NERF_GRID_OPTIM_RMSPROP * 10 + NERF_GRID_OPTIM_SGD);'])
    assert consts == {"consts": {"tv": _lib.NERF_GRID_TV_DENSITY * 10 + _lib.NERF_GRID_TV_SH,
                                 "optim": _lib.NERF_GRID_OPTIM_RMSPROP * 10 + _lib.NERF_GRID_OPTIM_SGD}}


def test_training_calls_refuse_bad_arguments_before_any_device_call():
    """Every refusal here comes before a handle is dereferenced: the grid and context pointers are fakes."""
    import nerf_projects_amd  # noqa: F401
    from nerf_projects_amd import _lib
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in _lib.EXPORTS
    fake = C.c_void_p(0x1000)
    err = lambda: lib.nerf_last_error().decode()      # noqa: E731
    opt, a = _lib.GridRenderOptions(), _lib.GridFusedArgs()
    opt.step_size, opt.background_brightness = 0.5, 1.0
    assert lib.nerf_grid_fused_backward(None, C.byref(opt), C.byref(a)) == -1 and "NULL grid" in err()
    assert lib.nerf_grid_fused_backward(fake, None, C.byref(a)) == -1 and "NULL" in err()
    assert lib.nerf_grid_fused_backward(fake, C.byref(opt), None) == -1 and "NULL" in err()
    a.struct_size -= 8
    assert lib.nerf_grid_fused_backward(fake, C.byref(opt), C.byref(a)) == -1 and "struct_size" in err()
    a = _lib.GridFusedArgs()
    opt.struct_size += 4
    assert lib.nerf_grid_fused_backward(fake, C.byref(opt), C.byref(a)) == -1 and "struct_size" in err()
    for field, obj_name, value, word in (("last_sample_opaque", "opt", 1, "last_sample_opaque"), ("randomize", "opt", 1, "randomize"),
                                         ("beta_loss", "a", 0.1, "beta_loss"), ("sparsity_loss", "a", 0.1, "sparsity_loss"),
                                         ("background_nlayers", "a", 4, "background")):
        opt, a = _lib.GridRenderOptions(), _lib.GridFusedArgs()
        opt.step_size, opt.background_brightness = 0.5, 1.0
        setattr(opt if obj_name == "opt" else a, field, value)
        assert lib.nerf_grid_fused_backward(fake, C.byref(opt), C.byref(a)) == -1, field
        assert word in err() and "not built" in err(), (field, err())
    opt, a = _lib.GridRenderOptions(), _lib.GridFusedArgs()
    opt.step_size, opt.background_brightness = 0.5, 1.0
    a.n_rays = 4      # and no pointers
    assert lib.nerf_grid_fused_backward(fake, C.byref(opt), C.byref(a)) == -1 and "required" in err()
    a.n_rays = -1
    assert lib.nerf_grid_fused_backward(fake, C.byref(opt), C.byref(a)) == -1 and "n_rays" in err()
    a.n_rays = 0
    assert lib.nerf_grid_fused_backward(fake, C.byref(opt), C.byref(a)) == 0      # zero rays: nothing is done

    tv = _lib.GridTvArgs()
    assert lib.nerf_grid_tv_grad(None, C.byref(tv)) == -1 and "NULL grid" in err()
    assert lib.nerf_grid_tv_grad(fake, None) == -1 and "NULL" in err()
    tv.struct_size = 0
    assert lib.nerf_grid_tv_grad(fake, C.byref(tv)) == -1 and "struct_size" in err()
    for field in ("ignore_edge", "ignore_last_z", "use_ndc"):
        tv = _lib.GridTvArgs()
        setattr(tv, field, 1)
        assert lib.nerf_grid_tv_grad(fake, C.byref(tv)) == -1 and "not built" in err(), field
    tv = _lib.GridTvArgs()
    tv.target = 2
    assert lib.nerf_grid_tv_grad(fake, C.byref(tv)) == -1 and "target" in err()
    tv = _lib.GridTvArgs()
    tv.count = 5      # and no grad / mask
    assert lib.nerf_grid_tv_grad(fake, C.byref(tv)) == -1 and "required" in err()

    op = _lib.GridOptimArgs()
    assert lib.nerf_grid_optim_step(None, C.byref(op)) == -1 and "NULL context" in err()
    assert lib.nerf_grid_optim_step(fake, None) == -1 and "NULL" in err()
    op.struct_size += 8
    assert lib.nerf_grid_optim_step(fake, C.byref(op)) == -1 and "struct_size" in err()
    op = _lib.GridOptimArgs()
    op.kind, op.cols = 7, 1
    assert lib.nerf_grid_optim_step(fake, C.byref(op)) == -1 and "kind" in err()
    op.kind, op.cols = 0, 0
    assert lib.nerf_grid_optim_step(fake, C.byref(op)) == -1 and "cols" in err()
    op.cols, op.rows = 3, 10      # and no pointers
    assert lib.nerf_grid_optim_step(fake, C.byref(op)) == -1 and "required" in err()
    op.rows = 0
    assert lib.nerf_grid_optim_step(fake, C.byref(op)) == 0


def test_grid_train_kernels_use_no_scratch_no_inline_assembly_and_no_compare_and_swap(tmp_path):
    text, asm, build = compile_kernels_to_asm(tmp_path, "grid_train_kernels.hip")
    assert "grid_train_kernels.hip" in build.SOURCES and "grid_train_api.cpp" in build.SOURCES
    assert any(h.endswith("grid_device.h") for h in build.HEADERS)
    for name, src in (("grid_train_kernels.hip", text), ("grid_device.h", open(os.path.join(build.CSRC, "grid_device.h")).read())):
        assert not re.search(r"\basm\b|__asm", src), name
    kernels = re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M)
    assert sum("grid_fused_kernel" in k for k in kernels) == 6 and len(kernels) == 9, kernels      # B in {9, 4, 1} x skip
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)
    assert len(sizes) == len(kernels) and all(int(s) == 0 for s in sizes), sizes
    assert not re.search(r"\bscratch_(load|store)", asm)
    assert "cmpswap" not in asm                                   # float adds are one hardware atomic each, no CAS loop
    assert len(re.findall(r"\bglobal_atomic_add_f32\b", asm)) > 0
    assert not re.search(r"global_atomic_add_f32[^\n]*\bsc0\b", asm)      # none returns the old value
    lds = re.findall(r"\.group_segment_fixed_size:\s*(\d+)", asm)
    assert all(int(s) == 0 for s in lds), lds
    vgprs = [int(v) for v in re.findall(r"\.vgpr_count:\s*(\d+)", asm)]
    print("vgprs per kernel:", dict(zip(kernels, vgprs)))
    assert max(vgprs) <= 80      # 6 waves per SIMD at basis_dim 9, 7 at 4 and 1
