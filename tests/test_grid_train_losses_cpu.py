"""Sparse voxel grid training with the beta and sparsity losses and the edge-aware TV, the parts that need no GPU: the numpy
restatement (tests/grid_train_losses_oracle.py) against the reference's recorded autograd gradients and loop
(tests/golden/grid_train_losses.npz) and against the restatement without the terms, the edge rule on a hand-made lattice, the
C ABI of the three entry points, and the generated code of csrc/grid_train_losses_kernels.hip."""
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
import grid_train_losses_oracle as GL  # noqa: E402
import grid_train_oracle as GT  # noqa: E402
from grid_testlib import assert_structs_match_c_header, compile_kernels_to_asm  # noqa: E402

RENDER = os.path.join(ROOT, "tests", "golden", "grid_render.npz")
TRAIN = os.path.join(ROOT, "tests", "golden", "grid_train.npz")
LOSSES = os.path.join(ROOT, "tests", "golden", "grid_train_losses.npz")
GRIDS = ("a", "b", "c", "d")
BACKGROUNDS = (("bg1", 1.0), ("bg0", 0.0))
SETTINGS = (("beta", 1, 0), ("sparsity", 0, 1), ("both", 1, 1))


def fixture_grid(z, name):
    return {"links": z[f"{name}_links"], "density_data": z[f"{name}_density"], "sh_data": z[f"{name}_sh"],
            "radius": z[f"{name}_radius"], "center": z[f"{name}_center"]}


def weights(f, name, setting):
    """(lambda_beta, lambda_sparsity) of a setting: the fixture's per-grid weights, each on or off"""
    lb, ls = f[f"{name}_weights"].tolist()
    on_b, on_s = {s: (b, k) for s, b, k in SETTINGS}[setting]
    return lb * on_b, ls * on_s


def grad_bars(f, t, name, tag, setting):
    """{key: (fp64 gradient, 3 x the reference's own fp32 - fp64 distance)}; the SH gradient does not depend on the weights
    and is grid_train.npz's"""
    key = f"{name}_{tag}_{setting}"
    return {"density": (f[f"{key}_grad_density64"].astype(np.float64), 3.0 * float(f[f"{key}_grad_density_d_ref"])),
            "sh": (t[f"{name}_{tag}_grad_sh64"].astype(np.float64), 3.0 * float(f[f"{key}_grad_sh_d_ref"]))}


@functools.lru_cache(maxsize=None)
def oracle_case(name, tag, setting):
    """(rgb, grad_density, grad_sh, mask, log_transmit) of the restatement at the PyTorch statement's setting (sigma_thresh = 0,
    stop_thresh = 0); computed once, shared by the CPU and the GPU test, read only. ``setting`` "off": both weights 0."""
    z, t, f = np.load(RENDER), np.load(TRAIN), np.load(LOSSES)
    lb, ls = (0.0, 0.0) if setting == "off" else weights(f, name, setting)
    o = z[f"{name}_origins"]
    out = GL.fused(fixture_grid(z, name), o, z[f"{name}_dirs"], t[f"{name}_rgb_gt"], beta_loss=lb / o.shape[0], sparsity_loss=ls,
                   sigma_thresh=0.0, stop_thresh=0.0, background_brightness=dict(BACKGROUNDS)[tag])
    for a in out:
        a.setflags(write=False)
    return out


def test_fixture_holds_arrays_only_and_is_small():
    assert os.path.getsize(LOSSES) < 1 << 20
    f, z, t = np.load(LOSSES), np.load(RENDER), np.load(TRAIN)      # (allow_pickle is off: arrays only)
    want = set()
    for name in GRIDS:
        want.add(f"{name}_weights")
        assert f[f"{name}_weights"].shape == (2,) and (f[f"{name}_weights"] > 0).all()
        for tag, _ in BACKGROUNDS:
            for setting, _, _ in SETTINGS:
                key = f"{name}_{tag}_{setting}"
                want |= {f"{key}_grad_density64", f"{key}_grad_density_d_ref", f"{key}_grad_sh_d_ref", f"{key}_share"}
                assert f[f"{key}_grad_density64"].shape == z[f"{name}_density"].shape and f[f"{key}_grad_density64"].dtype == np.float32
                if setting != "both":      # each term alone moves the density gradient by 10 % .. 90 % of its norm
                    assert 0.1 <= float(f[f"{key}_share"]) <= 0.9, key
    for name in ("b", "c"):
        want |= {f"{name}_loop_{k}" for k in ("loss32", "loss64", "density32", "density64", "sh32", "sh64", "mask64", "params")}
        assert f[f"{name}_loop_params"].tolist() == [0.95, 1e-8, 1e-2, 1.0]
        l32, l64 = f[f"{name}_loop_loss32"], f[f"{name}_loop_loss64"]
        assert l64.shape == (20,) and np.abs(l32 - l64).max() < 1e-3 * (l64[0] - l64[-1])
        # the terms moved the optimisation: far from the loop without them
        assert np.abs(f[f"{name}_loop_density64"] - t[f"{name}_loop_density64"]).max() > 1.0
    assert set(f.files) == want


@pytest.mark.parametrize("setting", [s for s, _, _ in SETTINGS])
@pytest.mark.parametrize("name", GRIDS)
def test_oracle_gradients_match_the_reference_autograd(name, setting):
    """Every entry within 3 x d_ref, the reference's own fp32 - fp64 distance; nothing is left out."""
    z, t, f = np.load(RENDER), np.load(TRAIN), np.load(LOSSES)
    g = fixture_grid(z, name)
    for tag, bg in BACKGROUNDS:
        rgb, gd, gs, mask, log_t = oracle_case(name, tag, setting)
        fwd, fwd_logt = GO.render(g, z[f"{name}_origins"], z[f"{name}_dirs"], sigma_thresh=0.0, stop_thresh=0.0, background_brightness=bg)
        assert np.array_equal(rgb, fwd) and np.array_equal(log_t, fwd_logt)      # the restatement walks the renderer's lattice
        touched = np.zeros(mask.shape, dtype=bool)
        for key, got in (("density", gd), ("sh", gs)):
            want, tol = grad_bars(f, t, name, tag, setting)[key]
            err = np.abs(got.astype(np.float64) - want)
            print(f"grid {name} {tag} {setting} d/d{key}: restatement vs fp64 autograd max {err.max():.3e} (bar {tol:.3e}, max |g| "
                  f"{np.abs(want).max():.3e})")
            assert err.max() <= tol, (name, tag, setting, key, int(err.argmax()), err.max(), tol)      # every entry
            touched |= (want != 0).any(-1)
        assert np.array_equal(mask != 0, touched), (name, tag, setting)
        # grad_sh and the touched rows do not depend on the weights: bit for bit those of the weights-off call
        _, gd0, gs0, mask0, _ = oracle_case(name, tag, "off")
        assert np.array_equal(gs, gs0) and np.array_equal(mask, mask0) and not np.array_equal(gd, gd0)


@pytest.mark.parametrize("name", ("b", "c", "d"))
def test_oracle_with_both_weights_zero_is_the_fused_restatement(name):
    z, t = np.load(RENDER), np.load(TRAIN)
    g = fixture_grid(z, name)
    o, d, gt = z[f"{name}_origins"], z[f"{name}_dirs"], t[f"{name}_rgb_gt"]
    skip = GO.skip_distances(g["links"])
    for kw in ({}, {"skip": skip}, {"step_size": 0.3, "near_clip": 2.0, "sigma_thresh": 0.5, "stop_thresh": 1e-2, "background_brightness": 0.5}):
        rgb, gd, gs, mask, _ = GL.fused(g, o, d, gt, **kw)
        rgb_f, gd_f, gs_f, mask_f = GT.fused(g, o, d, gt, **kw)
        assert np.array_equal(rgb, rgb_f) and np.array_equal(mask, mask_f) and mask.any()
        assert np.array_equal(gd, gd_f) and np.array_equal(gs, gs_f)      # bit for bit


def test_oracle_loss_terms_are_the_difference_of_on_and_off():
    """loss_terms_density (what the split-route test compares against) is the on - off difference of the restatement, to the
    fp32 rounding of d_sigma: at most a few ulp of the larger of the two sums per term."""
    z, t, f = np.load(RENDER), np.load(TRAIN), np.load(LOSSES)
    g = fixture_grid(z, "c")
    o, d = z["c_origins"], z["c_dirs"]
    lb, ls = weights(f, "c", "both")
    _, gd1, _, _, log_t = oracle_case("c", "bg1", "both")
    _, gd0, _, _, _ = oracle_case("c", "bg1", "off")
    terms = GL.loss_terms_density(g, o, d, lb / o.shape[0], ls, log_t, sigma_thresh=0.0, stop_thresh=0.0)
    err = np.abs((gd1.astype(np.float64) - gd0) - terms).max()
    assert np.abs(terms).max() > 0 and err <= 1e-5 * max(np.abs(gd1).max(), np.abs(gd0).max())


def numpy_loop(z, t, f, name):
    """the 20 iterations of the fixture through the restatement: losses (the MSE part), final tables, per-iteration masks"""
    g = fixture_grid(z, name)
    g["density_data"] = (np.float32(0.5) * g["density_data"]).astype(np.float32)
    g["sh_data"] = np.zeros_like(g["sh_data"])
    beta, eps, lr_sh, lr_sigma = f[f"{name}_loop_params"].tolist()
    lb, ls = f[f"{name}_weights"].tolist()
    o, d = z[f"{name}_origins"][:704], z[f"{name}_dirs"][:704]
    target = z[f"{name}_bg1_rgb64"][:704].astype(np.float32)
    rms_d, rms_s = np.zeros_like(g["density_data"]), np.zeros_like(g["sh_data"])
    losses, masks = [], []
    for k in t[f"{name}_loop_idx"]:
        rgb, gd, gs, mask, _ = GL.fused(g, o[k], d[k], target[k], beta_loss=lb / len(k), sparsity_loss=ls, sigma_thresh=0.0, stop_thresh=0.0)
        losses.append(float(((rgb.astype(np.float64) - target[k]) ** 2).mean()))
        GT.optim_step(g["density_data"], rms_d, gd, mask, "rmsprop", lr_sigma, beta, eps)
        GT.optim_step(g["sh_data"], rms_s, gs, mask, "rmsprop", lr_sh, beta, eps)
        masks.append(mask != 0)
    return np.array(losses), g["density_data"], g["sh_data"], np.stack(masks)


def loop_bars(f, name):
    """the rule of the existing loop test (test_grid_train_cpu.loop_bars) on this fixture"""
    l32, l64 = f[f"{name}_loop_loss32"], f[f"{name}_loop_loss64"]
    bars = {"loss": max(3.0 * float(np.abs(l32 - l64).max()), 1e-5 * float(l64[0]))}
    for key in ("density", "sh"):
        a32, a64 = f[f"{name}_loop_{key}32"].astype(np.float64), f[f"{name}_loop_{key}64"]
        bars[key] = max(3.0 * float(np.abs(a32 - a64).max()), 1e-5 * float(np.abs(a64).max()))
    return bars


@pytest.mark.parametrize("name", ("b", "c"))
def test_oracle_loop_matches_the_reference_loop(name):
    z, t, f = np.load(RENDER), np.load(TRAIN), np.load(LOSSES)
    losses, dens, sh, masks = numpy_loop(z, t, f, name)
    bars = loop_bars(f, name)
    l64 = f[f"{name}_loop_loss64"]
    print(f"grid {name}: loss {losses[0]:.5f} -> {losses[-1]:.5f}; vs fp64 max {np.abs(losses - l64).max():.2e} (bar {bars['loss']:.2e}); "
          f"density {np.abs(dens - f[name + '_loop_density64']).max():.2e} (bar {bars['density']:.2e}); "
          f"sh {np.abs(sh - f[name + '_loop_sh64']).max():.2e} (bar {bars['sh']:.2e})")
    assert np.abs(losses - l64).max() <= bars["loss"]
    assert np.abs(dens - f[f"{name}_loop_density64"]).max() <= bars["density"]
    assert np.abs(sh - f[f"{name}_loop_sh64"]).max() <= bars["sh"]
    want = np.unpackbits(f[f"{name}_loop_mask64"], axis=-1)[:, :masks.shape[1]].astype(bool)
    assert np.array_equal(masks, want)      # the touched rows of every iteration


# ---- the edge rule on a hand-made lattice ---------------------------------------------------------------------------------
def edge_lattice():
    """3 x 3 x 3, five kept nodes, one value column each (density and a single SH channel at basis_dim 1 x 3 columns):
         (0,0,0) row 0   the cell the literal `link == 0` test leaves out; its +x neighbour (1,0,0) is kept
         (1,0,0) row 1   kept, +x neighbour (2,0,0) EMPTY, +y (1,1,0) kept, +z (1,0,1) empty
         (1,1,0) row 2
         (2,2,2) row 3   on the last plane of every axis: all three neighbours out of range
         (0,1,1) empty, next to the kept (1,1,1) row 4 along +x
    """
    links = np.full((3, 3, 3), -1, dtype=np.int32)
    links[0, 0, 0], links[1, 0, 0], links[1, 1, 0], links[2, 2, 2], links[1, 1, 1] = 0, 1, 2, 3, 4
    links[2, 0, 0] = -5      # empty links need not be -1
    density = np.array([[3.0], [1.0], [2.5], [4.0], [0.75]], dtype=np.float32)
    sh = np.stack([density[:, 0] * s for s in (1.0, -2.0, 0.5)], -1).astype(np.float32)
    return {"links": links, "density_data": density, "sh_data": sh, "radius": np.ones(3, np.float32), "center": np.zeros(3, np.float32)}


def edge_cell(g, xyz, target="density", ignore_edge=True, start_dim=0, end_dim=None):
    """(grad, mask) of the one cell ``xyz`` with scale 1"""
    X, Y, Z = g["links"].shape
    table = g["density_data"] if target == "density" else g["sh_data"]
    grad, mask = np.zeros_like(table), np.zeros(table.shape[0], np.uint8)
    GL.tv_grad(g, target, (xyz[0] * Y + xyz[1]) * Z + xyz[2], 1, 1.0, grad, mask, start_dim, end_dim, ignore_edge)
    return grad, mask


def check_edge_cases(cell):
    """The four properties of the issue, on ``cell(g, xyz, ignore_edge) -> (grad [5, 1], mask [5])``: run on the restatement
    here and on the device in tests/test_grid_train_losses.py."""
    g = edge_lattice()
    f32 = np.float32
    # a kept node with an empty +x (and +z) neighbour receives nothing along x: only its kept +y neighbour pulls
    grad, mask = cell(g, (1, 0, 0), True)
    dy = f32(2.5) - f32(1.0)
    idelta = f32(1.0) / np.sqrt(f32(1e-9) + dy * dy)
    val = dy * f32(3.0 / 256.0)
    assert np.allclose(grad[:, 0], [0.0, -val * idelta, val * idelta, 0.0, 0.0], rtol=1e-6, atol=0) and mask.tolist() == [0, 1, 1, 0, 0]
    # ... whereas without the rule the empty neighbours count as 0 and pull the node's value down
    grad0, _ = cell(g, (1, 0, 0), False)
    assert grad0[1, 0] > grad[1, 0] + 1e-3
    # an empty cell next to a kept one still adds to it: own value 0, +x neighbour 0.75
    grad, mask = cell(g, (0, 1, 1), True)
    assert grad[4, 0] > 0 and mask.tolist() == [0, 0, 0, 0, 1] and not np.delete(grad, 4, axis=0).any()
    # the cell whose own link is row 0 adds nothing, although its +x neighbour is kept and differs
    grad, mask = cell(g, (0, 0, 0), True)
    assert not grad.any() and not mask.any()
    grad0, mask0 = cell(g, (0, 0, 0), False)
    assert grad0[0, 0] != 0 and grad0[1, 0] != 0 and mask0[0] and mask0[1]
    # a cell on the last plane treats the out-of-range neighbours as empty: differences 0, nothing added
    grad, mask = cell(g, (2, 2, 2), True)
    assert not grad.any() and not mask.any()
    grad0, mask0 = cell(g, (2, 2, 2), False)
    assert grad0[3, 0] > 0 and mask0.tolist() == [0, 0, 0, 1, 0]


def test_edge_rule_on_a_hand_made_lattice():
    check_edge_cases(lambda g, xyz, edge: edge_cell(g, xyz, "density", edge))
    # the SH table, one column of it: the same cells, the values scaled by -2
    g = edge_lattice()
    grad, mask = edge_cell(g, (1, 0, 0), "sh", True, 1, 2)
    assert grad[1, 1] > 0 > grad[2, 1] and not grad[:, [0, 2]].any() and mask.tolist() == [0, 1, 1, 0, 0]
    # with the flag off the restatement is the old one
    a, ma = np.zeros_like(g["sh_data"]), np.zeros(5, np.uint8)
    b, mb = np.zeros_like(g["sh_data"]), np.zeros(5, np.uint8)
    GL.tv_grad(g, "sh", 20, 27, 0.3, a, ma, ignore_edge=False)
    GT.tv_grad(g, "sh", 20, 27, 0.3, b, mb)
    assert np.array_equal(a, b) and np.array_equal(ma, mb) and a.any()


# ---- C ABI ------------------------------------------------------------------------------------------------------------
NEW_STRUCTS = {"nerf_grid_render_backward_losses_args": "GridRenderBackwardLossesArgs"}
NEW_SYMBOLS = ("nerf_grid_fused_backward_losses", "nerf_grid_render_backward_losses", "nerf_grid_tv_grad_edge")


def test_losses_struct_matches_a_c_compile_of_the_header(tmp_path):
    assert_structs_match_c_header(tmp_path, NEW_STRUCTS)


def test_losses_calls_refuse_bad_arguments_before_any_device_call():
    """Every refusal here comes before a handle is dereferenced: the grid pointer is a fake."""
    import nerf_projects_amd  # noqa: F401
    from nerf_projects_amd import _lib
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in _lib.EXPORTS
    fake = C.c_void_p(0x1000)
    err = lambda: lib.nerf_last_error().decode()      # noqa: E731
    buf = (C.c_float * 12)()
    ptr = C.addressof(buf)

    def options():
        opt = _lib.GridRenderOptions()
        opt.step_size, opt.background_brightness = 0.5, 1.0
        return opt

    # ---- nerf_grid_fused_backward_losses ----
    fn = lib.nerf_grid_fused_backward_losses
    opt, a = options(), _lib.GridFusedArgs()
    assert fn(None, C.byref(opt), C.byref(a)) == -1 and "NULL grid" in err()
    assert fn(fake, None, C.byref(a)) == -1 and "NULL" in err()
    assert fn(fake, C.byref(opt), None) == -1 and "NULL" in err()
    a.struct_size -= 8
    assert fn(fake, C.byref(opt), C.byref(a)) == -1 and "struct_size" in err()
    for field in ("beta_loss", "sparsity_loss"):
        for bad in (-0.1, float("nan"), float("inf"), -float("inf")):
            a = _lib.GridFusedArgs()
            setattr(a, field, bad)
            assert fn(fake, C.byref(opt), C.byref(a)) == -1 and field in err() and ">= 0" in err(), (field, bad, err())
    for field in ("last_sample_opaque", "randomize"):
        opt, a = options(), _lib.GridFusedArgs()
        setattr(opt, field, 1)
        assert fn(fake, C.byref(opt), C.byref(a)) == -1 and field in err() and "not built" in err(), field
    opt, a = options(), _lib.GridFusedArgs()
    a.background_nlayers = 4
    assert fn(fake, C.byref(opt), C.byref(a)) == -1 and "background" in err() and "not built" in err()
    a = _lib.GridFusedArgs()
    a.beta_loss, a.sparsity_loss, a.n_rays = 0.5, 0.25, 4      # accepted weights, and no pointers
    assert fn(fake, C.byref(opt), C.byref(a)) == -1 and "required" in err()
    a.n_rays = -1
    assert fn(fake, C.byref(opt), C.byref(a)) == -1 and "n_rays" in err()
    a.n_rays = 0
    assert fn(fake, C.byref(opt), C.byref(a)) == 0      # zero rays: nothing is done
    # the old entry keeps refusing, and says where the capability is
    assert lib.nerf_grid_fused_backward(fake, C.byref(opt), C.byref(a)) == -1
    assert "beta_loss" in err() and "not built" in err() and "nerf_grid_fused_backward_losses" in err()

    # ---- nerf_grid_render_backward_losses ----
    fn = lib.nerf_grid_render_backward_losses
    a, ls = _lib.GridRenderBackwardArgs(), _lib.GridRenderBackwardLossesArgs()
    assert fn(None, C.byref(opt), C.byref(a), C.byref(ls)) == -1 and "NULL grid" in err()
    assert fn(fake, None, C.byref(a), C.byref(ls)) == -1 and "NULL" in err()
    assert fn(fake, C.byref(opt), None, C.byref(ls)) == -1 and "NULL" in err()
    assert fn(fake, C.byref(opt), C.byref(a), None) == -1 and "nerf_grid_render_backward_losses_args is NULL" in err()
    ls.struct_size += 8
    assert fn(fake, C.byref(opt), C.byref(a), C.byref(ls)) == -1 and "struct_size" in err()
    ls = _lib.GridRenderBackwardLossesArgs()
    a.struct_size -= 8
    assert fn(fake, C.byref(opt), C.byref(a), C.byref(ls)) == -1 and "struct_size" in err()
    a = _lib.GridRenderBackwardArgs()
    for field in ("beta_loss", "sparsity_loss"):
        for bad in (-1e-3, float("nan"), float("inf")):
            ls = _lib.GridRenderBackwardLossesArgs()
            setattr(ls, field, bad)
            assert fn(fake, C.byref(opt), C.byref(a), C.byref(ls)) == -1 and field in err() and ">= 0" in err(), (field, bad)
    for field in ("last_sample_opaque", "randomize"):
        bad_opt = options()
        setattr(bad_opt, field, 1)
        assert fn(fake, C.byref(bad_opt), C.byref(a), C.byref(ls := _lib.GridRenderBackwardLossesArgs())) == -1 and field in err()
    ls = _lib.GridRenderBackwardLossesArgs()
    a.n_rays = 4      # and no pointers
    assert fn(fake, C.byref(opt), C.byref(a), C.byref(ls)) == -1 and "required" in err()
    a.origins = a.dirs = a.grad_rgb = ptr      # everything but the tape
    assert fn(fake, C.byref(opt), C.byref(a), C.byref(ls)) == -1 and "tape" in err()
    a.tape = a.grad_density = ptr
    ls.beta_loss = 0.5      # and no log_transmit
    assert fn(fake, C.byref(opt), C.byref(a), C.byref(ls)) == -1 and "log_transmit" in err()
    ls.log_transmit, a.grad_density, a.grad_sh = ptr, None, ptr      # a term and no density gradient to put it in
    assert fn(fake, C.byref(opt), C.byref(a), C.byref(ls)) == -1 and "grad_density" in err()
    ls.beta_loss, ls.sparsity_loss, ls.log_transmit = 0.0, 0.125, None      # the sparsity term alone needs no log_transmit ...
    assert fn(fake, C.byref(opt), C.byref(a), C.byref(ls)) == -1 and "grad_density" in err()      # ... but the gradient
    a.n_rays = (1 << 26) + 1
    assert fn(fake, C.byref(opt), C.byref(a), C.byref(ls)) == -1 and "n_rays" in err()
    a.n_rays = 0
    assert fn(fake, C.byref(opt), C.byref(a), C.byref(ls)) == 0      # zero rays: nothing is done

    # ---- nerf_grid_tv_grad_edge ----
    fn = lib.nerf_grid_tv_grad_edge
    tv = _lib.GridTvArgs()
    assert fn(None, C.byref(tv)) == -1 and "NULL grid" in err()
    assert fn(fake, None) == -1 and "NULL" in err()
    tv.struct_size = 0
    assert fn(fake, C.byref(tv)) == -1 and "struct_size" in err()
    for bad in (2, -1):
        tv = _lib.GridTvArgs()
        tv.ignore_edge = bad
        assert fn(fake, C.byref(tv)) == -1 and "ignore_edge" in err() and "0 or 1" in err(), bad
    for field in ("ignore_last_z", "use_ndc"):
        tv = _lib.GridTvArgs()
        tv.ignore_edge = 1
        setattr(tv, field, 1)
        assert fn(fake, C.byref(tv)) == -1 and "not built" in err(), field
    for edge in (0, 1):
        tv = _lib.GridTvArgs()
        tv.ignore_edge, tv.target = edge, 2
        assert fn(fake, C.byref(tv)) == -1 and "target" in err()
        tv.target, tv.scale = 0, float("nan")
        assert fn(fake, C.byref(tv)) == -1 and "scale" in err()
        tv.scale, tv.count = 1.0, 5      # and no grad / mask
        assert fn(fake, C.byref(tv)) == -1 and "required" in err()
    # the old entry keeps refusing, and says where the capability is
    tv = _lib.GridTvArgs()
    tv.ignore_edge = 1
    assert lib.nerf_grid_tv_grad(fake, C.byref(tv)) == -1 and "not built" in err() and "nerf_grid_tv_grad_edge" in err()


def test_python_refusals_that_need_no_device():
    import inspect

    import nerf_projects_amd as N
    for cls in (N.GridTrainer, N.BackgroundTrainer):
        sig = inspect.signature(cls.volume_render_fused)
        assert list(sig.parameters) == ["self", "rays", "rgb_gt", "randomize", "beta_loss", "sparsity_loss", "return_log_transmit"]
        assert [p.default for p in list(sig.parameters.values())[3:]] == [False, 0.0, 0.0, False]
        assert inspect.signature(cls.add_tv_grad).parameters["ignore_edge"].default is False
        step = inspect.signature(cls.train_step).parameters
        assert (step["lambda_beta"].default, step["lambda_sparsity"].default, step["tv_sh_ignore_edge"].default) == (0.0, 0.0, False)


def test_losses_kernels_use_no_scratch_no_inline_assembly_and_no_compare_and_swap(tmp_path):
    text, asm, build = compile_kernels_to_asm(tmp_path, "grid_train_losses_kernels.hip")
    assert "grid_train_losses_kernels.hip" in build.SOURCES
    assert any(h.endswith("grid_train_device.h") for h in build.HEADERS)
    for name, src in (("grid_train_losses_kernels.hip", text),
                      ("grid_train_device.h", open(os.path.join(build.CSRC, "grid_train_device.h")).read())):
        assert not re.search(r"\basm\b|__asm", src), name
    kernels = re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M)
    # fused and render backward with the terms: B in {9, 4, 1} x skip; one TV kernel with the edge rule
    assert sum("grid_fused_kernel" in k for k in kernels) == 6 and sum("grid_render_bwd_kernel" in k for k in kernels) == 6
    assert sum("grid_tv_grad_kernel" in k for k in kernels) == 1 and len(kernels) == 13, kernels
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)
    assert len(sizes) == len(kernels) and all(int(s) == 0 for s in sizes), sizes
    assert not re.search(r"\bscratch_(load|store)", asm)
    assert "cmpswap" not in asm                                   # float adds are one hardware atomic each, no CAS loop
    assert len(re.findall(r"\bglobal_atomic_add_f32\b", asm)) > 0
    assert not re.search(r"global_atomic_add_f32[^\n]*\bsc0\b", asm)      # none returns the old value
    lds = re.findall(r"\.group_segment_fixed_size:\s*(\d+)", asm)
    assert all(int(s) == 0 for s in lds), lds
    vgprs = dict(zip(kernels, (int(v) for v in re.findall(r"\.vgpr_count:\s*(\d+)", asm))))
    print("vgprs per kernel:", vgprs)
    assert max(vgprs.values()) <= 80      # the occupancy of the kernels without the terms: 6 waves per SIMD at basis_dim 9
