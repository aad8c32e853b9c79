"""Training the background layers, without a GPU: the numpy restatement (tests/grid_background_train_oracle.py) against the
autograd gradients of tests/golden/grid_background_train.npz and against fp64 autograd of the TV statement, the optimiser
per column against grid_train_oracle.optim_step, the C ABI (structs, argument checks without a device) and the generated code.
What the GPU tests (tests/test_grid_background_train.py) compare the kernels with is computed here once and shared."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import grid_background_oracle as BO
import grid_background_train_oracle as BT
import grid_oracle as GO
import grid_train_oracle as GT
from grid_testlib import ROOT, assert_structs_match_c_header, compile_kernels_to_asm

GOLDEN = os.path.join(ROOT, "tests", "golden", "grid_background_train.npz")
F = np.float32
RESO = (12, 14, 10)
N_SETTINGS = 8


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def fixture_grid(z):
    return {"links": z["links"], "density_data": z["density"], "sh_data": z["sh"], "radius": z["radius"], "center": z["center"]}


def fixture_background(z, nl):
    return {"links": z[f"bg{int(nl)}_links"], "data": z[f"bg{int(nl)}_data"]}


def grad_bar(z, j, key):
    """3x the reference's own fp32 - fp64 distance, and no tighter than 1e-5 of the table's largest entry (the project's bar:
    grad_bar of tests/test_grid_train_cpu.py)"""
    want = z[f"set{j}_grad_{key}64"].astype(np.float64)
    return want, max(3.0 * float(z[f"set{j}_grad_{key}_d_ref"]), 1e-5 * float(np.abs(want).max()))


@functools.lru_cache(maxsize=None)
def restated(j, sigma_thresh=0.0):
    """forward_backward of setting j in the fp32 restatement: computed once, shared (read only)"""
    z = fixture()
    nl, step, stop, bright = z["settings"][j]
    out = BT.forward_backward(fixture_grid(z), fixture_background(z, nl), z["origins"], z["dirs"], z["rgb_gt"], float(step),
                              sigma_thresh, float(stop), float(bright))
    for a in out.values():
        a.setflags(write=False)
    return out


def test_fixture_holds_arrays_only_and_is_small():
    assert os.path.getsize(GOLDEN) < 1 << 20
    z = np.load(GOLDEN, allow_pickle=False)
    for k in z.files:
        assert z[k].dtype.kind in "fiub", k
    assert z["settings"].shape == (N_SETTINGS, 4) and z["origins"].shape == (512, 3)
    assert tuple(z["links"].shape) == RESO
    assert {int(s[0]) for s in z["settings"]} == {2, 5, 8} and {float(s[3]) for s in z["settings"]} == {0.0, 1.0}


@pytest.mark.parametrize("j", range(N_SETTINGS))
def test_fp64_restatement_of_the_backward_is_the_autograd_gradient(j):
    """The reference's `accum` form, restated in fp64 and fed with the fp64 foreground, is the derivative of the forward that
    tests/test_grid_background_cpu.py pins: 1e-10 of the table's largest entry."""
    z = fixture()
    nl, step, stop, bright = z["settings"][j]
    g, bg = fixture_grid(z), fixture_background(z, nl)
    og, dg, _, ds, _, _, ok = GO.ray_setup(g, z["origins"], z["dirs"])
    assert np.array_equal(ok, z["setup_ok"])
    n = z["origins"].shape[0]
    logt64, rgb64 = z[f"set{j}_fg_logt64"], z[f"set{j}_rgb64"]
    args = (og, dg, ds, ok, RESO, bg)
    rgb_bg, _, _, tb = BT.taped(*args, np.zeros((n, 3)), logt64, np.zeros((n, 3)), float(step), float(stop), float(bright), T=np.float64)
    g64 = (rgb64 - z["rgb_gt"].astype(np.float64)) * (2.0 / (3.0 * n))
    got, mask = BT.backward(*args, g64, logt64, tb, float(step), float(stop), T=np.float64)
    want = z[f"set{j}_grad_background64"]
    err, big = float(np.abs(got - want).max()), float(np.abs(want).max())
    print(f"setting {j}: fp64 restatement vs fp64 autograd max {err:.3e} = {err / big:.2e} of the largest entry")
    assert big > 0 and err <= 1e-10 * big
    assert not got[mask == 0].any()


@pytest.mark.parametrize("j", range(N_SETTINGS))
def test_fp32_restatement_sits_within_the_bar_of_the_autograd_gradients(j):
    z = fixture()
    r = restated(j)
    err_rgb = float(np.abs(r["rgb"].astype(np.float64) - z[f"set{j}_rgb64"]).max())
    assert err_rgb <= max(3.0 * float(z[f"set{j}_rgb_d_ref"]), 1e-5)
    for key in ("density", "sh", "background"):
        want, tol = grad_bar(z, j, key)
        got = r[f"grad_{key}"].astype(np.float64).reshape(want.shape)
        err = float(np.abs(got - want).max())
        print(f"setting {j} d/d{key}: restatement vs fp64 autograd max {err:.3e} (bar {tol:.3e}, max |g| {np.abs(want).max():.3e})")
        assert err <= tol, key
    # the mask covers every entry that received something; left-alone and non-finite rays gave nothing
    assert not r["grad_background"][r["mask_background"] == 0].any()
    assert ((r["fg_log_transmit"] < -25) & z["setup_ok"]).sum() >= 16


def test_restatement_accumulates_and_the_taped_pass_is_the_forward():
    z = fixture()
    j = 3
    nl, step, stop, bright = z["settings"][j]
    g, bg = fixture_grid(z), fixture_background(z, nl)
    r = restated(j)
    state = {k: r[k].copy() for k in ("grad_density", "grad_sh", "mask", "grad_background", "mask_background")}
    r2 = BT.forward_backward(g, bg, z["origins"], z["dirs"], z["rgb_gt"], float(step), 0.0, float(stop), float(bright), state=state)
    for key in ("grad_density", "grad_sh", "grad_background"):
        assert np.abs(r2[key] - 2 * r[key]).max() <= 1e-5 * np.abs(r[key]).max()
    # rgb and log_transmit of the taped pass are grid_background_oracle.background_pass's, bit for bit
    fg_rgb, fg_logt = GO.render(g, z["origins"], z["dirs"], step_size=float(step), sigma_thresh=0.0, stop_thresh=float(stop),
                                background_brightness=0.0)
    og, dg, _, ds, _, _, ok = GO.ray_setup(g, z["origins"], z["dirs"])
    rgb, logt = BO.background_pass(og, dg, ds, ok, RESO, bg, fg_rgb, fg_logt, float(step), float(stop), float(bright))
    assert np.array_equal(rgb, r["rgb"], equal_nan=True) and np.array_equal(logt, r["log_transmit"], equal_nan=True)


# ---- a training loop ---------------------------------------------------------------------------------------------------
def loop_bars(z):
    """as loop_bars of tests/test_grid_train_cpu.py: 3x the distance of the fp32 from the fp64 autograd loop, and no tighter
    than 1e-5 of the first loss / of the table's largest entry"""
    l32, l64 = z["loop_loss32"], z["loop_loss64"]
    bars = {"loss": max(3.0 * float(np.abs(l32 - l64).max()), 1e-5 * float(l64[0]))}
    for key in ("density", "sh", "background"):
        a32, a64 = z[f"loop_{key}32"].astype(np.float64), z[f"loop_{key}64"]
        bars[key] = max(3.0 * float(np.abs(a32 - a64).max()), 1e-5 * float(np.abs(a64).max()))
    return bars


LOOP_SETTING = 4


@functools.lru_cache(maxsize=None)
def restated_loop():
    """the fixture's 20 iterations in the fp32 restatement: the losses, the three final tables and the starting tables"""
    z = fixture()
    nl, step, stop, bright = z["settings"][LOOP_SETTING]
    beta, eps, lr_sh, lr_sigma, lr_sigma_bg, lr_color_bg = (float(v) for v in z["loop_params"])
    g = dict(fixture_grid(z), density_data=(0.5 * np.minimum(z["density"], 2.0)).astype(F), sh_data=np.zeros_like(z["sh"]))
    bg = {"links": fixture_background(z, nl)["links"], "data": (0.5 * fixture_background(z, nl)["data"]).astype(F)}
    out = dict(setting=LOOP_SETTING, density0=g["density_data"].copy(), sh0=g["sh_data"].copy(), background0=bg["data"].copy())
    rms = [np.zeros_like(g["density_data"]), np.zeros_like(g["sh_data"]), np.zeros_like(bg["data"])]
    target = z[f"set{LOOP_SETTING}_rgb64"].astype(F)
    losses = []
    for k in z["loop_idx"]:
        r = BT.forward_backward(g, bg, z["origins"][k], z["dirs"][k], target[k], float(step), 0.0, float(stop), float(bright))
        losses.append(float(((r["rgb"].astype(np.float64) - target[k]) ** 2).mean()))
        GT.optim_step(g["density_data"], rms[0], r["grad_density"], r["mask"], "rmsprop", lr_sigma, beta, eps)
        GT.optim_step(g["sh_data"], rms[1], r["grad_sh"], r["mask"], "rmsprop", lr_sh, beta, eps)
        BT.optim_step(bg["data"], rms[2], r["grad_background"], r["mask_background"], "rmsprop", lr_sigma_bg, lr_color_bg, beta, eps)
    out.update(loss=np.array(losses), density=g["density_data"], sh=g["sh_data"], background=bg["data"])
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def test_restated_loop_follows_the_autograd_loop():
    z = fixture()
    bars, got = loop_bars(z), restated_loop()
    err = float(np.abs(got["loss"] - z["loop_loss64"]).max())
    print(f"loop loss {got['loss'][0]:.5f} -> {got['loss'][-1]:.5f}: restatement vs fp64 autograd {err:.3e} (bar {bars['loss']:.3e})")
    assert got["loss"][-1] < 0.5 * got["loss"][0] and err <= bars["loss"]
    for key in ("density", "sh", "background"):
        e = float(np.abs(got[key].astype(np.float64) - z[f"loop_{key}64"]).max())
        print(f"loop final {key}: restatement vs fp64 autograd {e:.3e} (bar {bars[key]:.3e})")
        assert e <= bars[key], key


# ---- TV --------------------------------------------------------------------------------------------------------------
def tv_background():
    """8 x 4 texels (R = 4), L = 3: empty texels (on both seams too), rows permuted, a plateau texel column"""
    rng = np.random.default_rng(8403)
    R, L = 4, 3
    kept = rng.random((2 * R, R)) < 0.75
    kept[0, 0] = kept[2 * R - 1, 1] = kept[3, R - 1] = kept[3, 0] = True
    kept[2 * R - 1, 2] = kept[5, R - 1] = False
    n = int(kept.sum())
    links = np.full((2 * R, R), -1, np.int32)
    links[kept] = rng.permutation(n).astype(np.int32)
    data = rng.normal(0.0, 1.5, (n, L, 4)).astype(F)
    return {"links": links, "data": data}


def tv_grad_fp64(bg, scale_sigma, scale_color):
    """The TV statement over all cells, independent of the restatement: fp64 autograd. v = the [2R, R, L, 4] volume, 0 at texels
    without a row; dx, dy to the wrapped neighbours, dz to the next layer where the texel has a row and a next layer, else
    (0 - v) for sigma and 0 for the colours; inv = scale_c / sqrt(1e-9 + dx^2 + dy^2 + dz^2) held constant; the gradient of
    sum(0.5 inv (s_x dx^2 + s_y dy^2 + s_z dz^2)), s = (2R, R, L) / 256 - where the differences reach a cell that cannot
    receive (no row, or no next layer) the other end is held constant."""
    import torch
    links, data = bg["links"], bg["data"]
    R2, R = links.shape
    L = data.shape[1]
    t = torch.tensor(data.astype(np.float64), requires_grad=True)
    lk = torch.from_numpy(links.astype(np.int64))
    has = (lk >= 0)
    v = torch.where(has[..., None, None], t[lk.clamp_min(0)], torch.zeros((), dtype=torch.float64))      # [2R, R, L, 4]
    dx = torch.roll(v, -1, 0) - v
    dy = torch.roll(v, -1, 1) - v
    nxt = torch.cat([v[:, :, 1:], torch.zeros_like(v[:, :, :1])], 2)
    edge = v.detach().clone()
    edge[..., 3] = 0.0
    last = torch.zeros(L, dtype=torch.bool)
    last[L - 1] = True
    no_next = (~has)[..., None, None] | last[None, None, :, None]
    dz = torch.where(no_next, edge, nxt) - v
    scale = torch.tensor([scale_color] * 3 + [scale_sigma], dtype=torch.float64)
    inv = (scale / torch.sqrt(1e-9 + dx * dx + dy * dy + dz * dz)).detach()
    sx, sy, sz = (float(F(s) * F(1.0 / 256.0)) for s in (R2, R, L))
    (0.5 * inv * (sx * dx * dx + sy * dy * dy + sz * dz * dz)).sum().backward()
    return t.grad.numpy()


TV_SCALES = (0.37, 0.011)      # sigma, colour


@functools.lru_cache(maxsize=None)
def tv_case():
    """(background, cells, fp64 gradient, restated gradient, restated mask): all 96 cells from a start that wraps"""
    bg = tv_background()
    cells = bg["links"].size * bg["data"].shape[1]
    ss, sc = F(TV_SCALES[0] / cells), F(TV_SCALES[1] / cells)
    want = tv_grad_fp64(bg, float(ss), float(sc))
    grad, mask = np.zeros_like(bg["data"]), np.zeros(bg["data"].shape[:2], np.uint8)
    BT.tv_grad(bg, cells - 7, cells, ss, sc, grad, mask)
    for a in (want, grad, mask):
        a.setflags(write=False)
    return bg, cells, want, grad, mask


def test_tv_restatement_matches_the_fp64_autograd_statement():
    """The bar, 1e-5 of the largest entry of a channel's kind: an entry is the sum of at most 7 terms of about 6 fp32 roundings
    each (the bar of the foreground's TV test)."""
    bg, cells, want, grad, mask = tv_case()
    assert cells == 96 and (bg["links"] < 0).any()
    for sl in (slice(0, 3), slice(3, 4)):
        big = float(np.abs(want[..., sl]).max())
        err = float(np.abs(grad[..., sl].astype(np.float64) - want[..., sl]).max())
        print(f"tv channels {sl}: restatement vs fp64 autograd max {err:.3e} = {err / big:.2e} of the largest entry")
        assert big > 0 and err <= 1e-5 * big
    assert np.array_equal(mask != 0, (want != 0).any(-1))
    # the last-layer rule: a colour's dz is 0 there, sigma's is (0 - v). Every texel is the same row: dx = dy = 0.
    L = bg["data"].shape[1]
    one = np.zeros_like(bg["data"])
    m = np.zeros(bg["data"].shape[:2], np.uint8)
    lk = int(bg["links"][0, 0])
    flat = (0 * bg["links"].shape[1] + 0) * L + (L - 1)
    alone = {"links": np.full_like(bg["links"], lk), "data": bg["data"]}
    BT.tv_grad(alone, flat, 1, F(1.0), F(1.0), one, m)
    assert not one[lk, L - 1, :3].any() and one[lk, L - 1, 3] != 0 and m.sum() == 1


def test_optimiser_matches_the_foreground_restatement_per_column_bit_for_bit():
    rng = np.random.default_rng(77)
    cap, L = 9, 3
    for kind in ("rmsprop", "sgd"):
        data = rng.normal(0, 1, (cap, L, 4)).astype(F)
        rms = (rng.random((cap, L, 4)) < 0.5).astype(F) * rng.random((cap, L, 4)).astype(F)
        grad = rng.normal(0, 1e-2, (cap, L, 4)).astype(F)
        grad[1, 1, 2], grad[2, 0, 3], grad[3, 2, 0] = np.nan, np.inf, F(1e-30)
        mask = (rng.random((cap, L)) < 0.7).astype(np.uint8)
        mask[0, 0], mask[1, 1] = 0, 5
        d0, r0 = data.copy(), rms.copy()
        BT.optim_step(data, rms, grad, mask, kind, 0.5, 1e-2)
        for c in range(4):
            dc, rc = d0[..., c].reshape(-1, 1).copy(), r0[..., c].reshape(-1, 1).copy()
            GT.optim_step(dc, rc, grad[..., c].reshape(-1, 1), mask.reshape(-1), kind, 0.5 if c == 3 else 1e-2)
            assert np.array_equal(dc.reshape(cap, L), data[..., c], equal_nan=True)
            assert np.array_equal(rc.reshape(cap, L), rms[..., c], equal_nan=True)
        assert np.array_equal(data[0, 0], d0[0, 0]) and np.array_equal(rms[0, 0], r0[0, 0])      # masked off
        assert data[1, 1, 2] == F(-1e9)      # a NaN gradient lands on minval


# ---- C ABI ------------------------------------------------------------------------------------------------------------
NEW_STRUCTS = {"nerf_grid_background_taped_args": "GridBackgroundTapedArgs",
               "nerf_grid_background_backward_args": "GridBackgroundBackwardArgs",
               "nerf_grid_background_tv_args": "GridBackgroundTvArgs",
               "nerf_grid_background_optim_args": "GridBackgroundOptimArgs"}
NEW_SYMBOLS = ("nerf_grid_background_rays_taped", "nerf_grid_background_backward", "nerf_grid_background_tv_grad",
               "nerf_grid_background_optim_step")


def test_structs_match_a_c_compile_of_the_header(tmp_path):
    assert assert_structs_match_c_header(tmp_path, NEW_STRUCTS) == {}


def test_calls_refuse_bad_arguments_before_any_device_call():
    """Every refusal here comes before a handle is dereferenced: the grid and context pointers are fakes."""
    import nerf_projects_amd  # noqa: F401
    from nerf_projects_amd import _lib
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in _lib.EXPORTS
    fake = C.c_void_p(0x1000)
    buf = (C.c_double * 8)()
    p, q = C.addressof(buf), C.addressof(buf) + 32
    err = lambda: lib.nerf_last_error().decode()      # noqa: E731

    def options():
        o = _lib.GridRenderOptions()
        o.step_size, o.background_brightness = 0.5, 1.0
        return o

    for fn, cls in ((lib.nerf_grid_background_rays_taped, _lib.GridBackgroundTapedArgs),
                    (lib.nerf_grid_background_backward, _lib.GridBackgroundBackwardArgs)):
        a = cls()
        assert fn(None, C.byref(options()), C.byref(a)) == -1 and "NULL grid" in err()
        assert fn(fake, None, C.byref(a)) == -1 and "NULL" in err()
        assert fn(fake, C.byref(options()), None) == -1 and "NULL" in err()
        a.struct_size -= 8
        assert fn(fake, C.byref(options()), C.byref(a)) == -1 and "struct_size" in err()
        for field in ("randomize", "last_sample_opaque"):
            o = options()
            setattr(o, field, 1)
            assert fn(fake, C.byref(o), C.byref(cls())) == -1 and field in err() and "not built" in err()
        a = cls()
        a.n_rays = -1
        assert fn(fake, C.byref(options()), C.byref(a)) == -1 and "n_rays" in err()
        a.n_rays = 4      # and no pointers
        assert fn(fake, C.byref(options()), C.byref(a)) == -1 and "origins" in err()
        a.origins = a.dirs = p
        assert fn(fake, C.byref(options()), C.byref(a)) == -1 and "required" in err()
        a.n_rays = 0
        assert fn(fake, C.byref(options()), C.byref(a)) == 0      # zero rays: nothing is done
    a = _lib.GridBackgroundTapedArgs()
    a.n_rays, a.origins, a.dirs, a.rgb, a.tape, a.tape_background = 4, p, p, p, p, p
    a.log_transmit = a.log_transmit_out = q
    assert lib.nerf_grid_background_rays_taped(fake, C.byref(options()), C.byref(a)) == -1 and "another array" in err()
    for field in ("sparsity_loss", "beta_loss"):
        b = _lib.GridBackgroundBackwardArgs()
        setattr(b, field, 0.1)
        assert lib.nerf_grid_background_backward(fake, C.byref(options()), C.byref(b)) == -1
        assert field in err() and "not built" in err()

    tv = _lib.GridBackgroundTvArgs()
    assert lib.nerf_grid_background_tv_grad(None, C.byref(tv)) == -1 and "NULL grid" in err()
    assert lib.nerf_grid_background_tv_grad(fake, None) == -1 and "NULL" in err()
    tv.struct_size = 0
    assert lib.nerf_grid_background_tv_grad(fake, C.byref(tv)) == -1 and "struct_size" in err()
    tv = _lib.GridBackgroundTvArgs()
    tv.scale_sigma = float("inf")
    assert lib.nerf_grid_background_tv_grad(fake, C.byref(tv)) == -1 and "finite" in err()
    tv = _lib.GridBackgroundTvArgs()
    tv.scale_color = float("nan")
    assert lib.nerf_grid_background_tv_grad(fake, C.byref(tv)) == -1 and "finite" in err()
    tv = _lib.GridBackgroundTvArgs()
    tv.count = 5      # and no grad / mask
    assert lib.nerf_grid_background_tv_grad(fake, C.byref(tv)) == -1 and "required" in err()

    op = _lib.GridBackgroundOptimArgs()
    assert lib.nerf_grid_background_optim_step(None, C.byref(op)) == -1 and "NULL context" in err()
    assert lib.nerf_grid_background_optim_step(fake, None) == -1 and "NULL" in err()
    op.struct_size += 8
    assert lib.nerf_grid_background_optim_step(fake, C.byref(op)) == -1 and "struct_size" in err()
    op = _lib.GridBackgroundOptimArgs()
    op.kind = 7
    assert lib.nerf_grid_background_optim_step(fake, C.byref(op)) == -1 and "kind" in err()
    op.kind, op.rows = 0, -1
    assert lib.nerf_grid_background_optim_step(fake, C.byref(op)) == -1 and "rows" in err()
    op.rows = (1 << 35) + 1
    assert lib.nerf_grid_background_optim_step(fake, C.byref(op)) == -1 and "rows" in err()
    op.rows = 10      # and no pointers
    assert lib.nerf_grid_background_optim_step(fake, C.byref(op)) == -1 and "required" in err()
    op.data = op.grad = op.mask = p      # RMSProp without rms
    assert lib.nerf_grid_background_optim_step(fake, C.byref(op)) == -1 and "required" in err()
    op.rms, op.lr_sigma = p, float("nan")
    assert lib.nerf_grid_background_optim_step(fake, C.byref(op)) == -1 and "NaN" in err()
    op.rows, op.lr_sigma = 0, 1.0
    assert lib.nerf_grid_background_optim_step(fake, C.byref(op)) == 0


# ---- generated code -----------------------------------------------------------------------------------------------------
def test_kernels_use_no_scratch_no_lds_no_inline_assembly_and_no_compare_and_swap(tmp_path):
    text, asm, build = compile_kernels_to_asm(tmp_path, "grid_background_train_kernels.hip")
    assert "grid_background_train_kernels.hip" in build.SOURCES and "grid_background_train_api.cpp" in build.SOURCES
    assert any(h.endswith("grid_background_device.h") for h in build.HEADERS)
    header = open(os.path.join(build.CSRC, "grid_background_device.h")).read()
    for name, src in (("grid_background_train_kernels.hip", text), ("grid_background_device.h", header)):
        assert not re.search(r"\basm\b|__asm", src), name
        assert not re.search(r"^\s*#\s*if", src.replace("#pragma once", ""), re.M), name      # no compile-time switches
    # the forward marches with the same header
    assert '#include "grid_background_device.h"' in open(os.path.join(build.CSRC, "grid_background_kernels.hip")).read()
    kernels = re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M)
    assert len(kernels) == 5, kernels      # taped, backward, tv, optimiser x 2
    assert not re.search(r"\bscratch_(load|store)", asm)
    assert "cmpswap" not in asm                                   # float adds are one hardware atomic each, no CAS loop
    assert len(re.findall(r"\bglobal_atomic_add_f32\b", asm)) >= 1 + 4      # the backward (one per lane) and the four TV terms
    assert not re.search(r"global_atomic_add_f32[^\n]*\bsc0\b", asm)      # none returns the old value
    assert re.search(r"\bglobal_store_byte\b", asm)               # the mask: plain byte stores
    # the compiler's own remark: scratch, LDS and registers per kernel
    path = os.path.join(build.CSRC, "grid_background_train_kernels.hip")
    cmd = [build.hipcc()] + build.FLAGS + build.VGPR_FORM + ["-I", os.path.join(ROOT, "include"), "-I", build.CSRC, "--cuda-device-only",
                                                              "-Rpass-analysis=kernel-resource-usage", "-c", path, "-o", str(tmp_path / "k.o")]
    remark = subprocess.run(cmd, check=True, cwd=tmp_path, capture_output=True, text=True).stderr
    names = re.findall(r"Function Name: (\S+)", remark)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", remark)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", remark)]
    vgprs = [int(v) for v in re.findall(r"\bVGPRs: (\d+)", remark)]
    print("vgprs per kernel:", dict(zip(names, vgprs)))
    assert len(names) == 5 and len(scratch) == 5 and len(lds) == 5 and len(vgprs) == 5
    assert all(s == 0 for s in scratch) and all(v == 0 for v in lds)
    assert max(vgprs) <= 96      # 5 waves per SIMD for the two marching kernels
