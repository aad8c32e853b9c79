"""Sparse voxel grid training with the beta and sparsity losses and the edge-aware TV on the GPU (include/nerf_mi355x.h,
"Sparse voxel grid: training with the beta and sparsity losses"): GridTrainer.volume_render_fused against the reference's
recorded autograd gradients and RMSProp loop (tests/golden/grid_train_losses.npz) and against the numpy restatement
(tests/grid_train_losses_oracle.py, checked against the same fixture in tests/test_grid_train_losses_cpu.py) off that setting;
BackgroundTrainer.volume_render_fused (the split route); add_tv_grad(ignore_edge=True); and the refusals that stay.
Needs a real MI355X: run with ``pytest -m gpu``."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import grid_oracle as GO
import grid_train_losses_oracle as GL
import test_grid_background_train as TB
from test_grid import cpu, gpu, make_grid, set_opt
from test_grid_background_train_cpu import fixture as bg_fixture, fixture_grid as bg_fixture_grid
from test_grid_train import assert_matches_restatement
from test_grid_train_losses_cpu import (BACKGROUNDS, GRIDS, LOSSES, RENDER, SETTINGS, TRAIN, check_edge_cases, fixture_grid, grad_bars,
                                        loop_bars, weights)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def N():
    import nerf_projects_amd as pkg
    return pkg


def run_losses(N, grid, trainer, o, d, gt, lambda_beta, lambda_sparsity):
    """zero_grad + volume_render_fused: (rgb, log_transmit, grad_density, grad_sh, mask) as numpy; rgb and log_transmit are
    the renderer's bits"""
    rays = N.Rays(gpu(o), gpu(d))
    trainer.zero_grad()
    rgb, logt = trainer.volume_render_fused(rays, gpu(gt), beta_loss=lambda_beta, sparsity_loss=lambda_sparsity, return_log_transmit=True)
    want_rgb, want_logt = grid.volume_render(rays, return_log_transmit=True)
    assert torch.equal(rgb, want_rgb) and torch.equal(logt, want_logt)      # bit-identical to the renderer
    return cpu(rgb).copy(), cpu(logt).copy(), cpu(trainer.grad_density).copy(), cpu(trainer.grad_sh).copy(), cpu(trainer.mask).copy()


# ---- 1. the reference's gradients ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", [s for s, _, _ in SETTINGS])
@pytest.mark.parametrize("name", GRIDS)
def test_volume_render_fused_against_the_reference_autograd(N, name, setting):
    """Every entry of grad_density and grad_sh within 3 x d_ref, the reference's own fp32 - fp64 distance."""
    z, t, f = np.load(RENDER), np.load(TRAIN), np.load(LOSSES)
    g = fixture_grid(z, name)
    o, d, gt = z[f"{name}_origins"], z[f"{name}_dirs"], t[f"{name}_rgb_gt"]
    lb, ls = weights(f, name, setting)
    grid = make_grid(N, g)
    trainer = N.GridTrainer(grid)
    failures = []
    for accelerated in (False, True):
        if accelerated:
            grid.accelerate()
        for tag, bg in BACKGROUNDS:
            set_opt(grid, bg, 0.5, 0.0, 0.0, 0.0)
            label = f"grid {name} {tag} {setting} {'accelerated' if accelerated else 'plain'}"
            _, _, gd, gs, mask = run_losses(N, grid, trainer, o, d, gt, lb, ls)
            touched = np.zeros(grid.capacity, dtype=bool)
            for key, got in (("density", gd), ("sh", gs)):
                want, tol = grad_bars(f, t, name, tag, setting)[key]
                err = np.abs(got.astype(np.float64) - want)
                print(f"{label} d/d{key}: GPU vs fp64 autograd max {err.max():.3e} (bar {tol:.3e}, max |g| {np.abs(want).max():.3e})")
                if not (np.isfinite(got).all() and err.max() <= tol):
                    failures.append((label, key, int(err.argmax()), float(err.max()), tol))
                touched |= (want != 0).any(-1)
            assert np.array_equal(mask != 0, touched), label
            # grad_sh is unaffected by the weights, to rounding of the sums, against the weights-off call
            trainer.zero_grad()
            trainer.forward_backward(N.Rays(gpu(o), gpu(d)), gpu(gt))
            gs0, gd0 = cpu(trainer.grad_sh), cpu(trainer.grad_density)
            assert np.abs(gs.astype(np.float64) - gs0).max() <= 1e-5 * np.abs(gs0).max(), label
            assert np.array_equal(cpu(trainer.mask), mask) and np.abs(gd - gd0).max() > 1e-3 * np.abs(gd0).max(), label
    assert not failures, failures


# ---- 2. off the recorded setting, against the restatement -------------------------------------------------------------
RESTATED_CASES = {
    "default": dict(),                                                       # stop_thresh 1e-7, sigma_thresh 1e-10
    "stop": dict(stop_thresh=0.05),                                          # rays that stop: T_in = 0, c_beta = beta_loss
    "sigma": dict(sigma_thresh=2.0, stop_thresh=0.05, background_brightness=0.5),
    "step": dict(step_size=0.3),
}
N_RESTATED = 701      # not a multiple of the rays of a wavefront (2 / 4 / 16 at basis_dim 9 / 4 / 1), more than one block


@functools.lru_cache(maxsize=None)
def restated_case(name, case):
    """(o, d, gt, lambda_beta, lambda_sparsity, GL.fused's result): 699 fixture rays, one that misses the box, one with a zero
    direction; computed once, read only"""
    z, t, f = np.load(RENDER), np.load(TRAIN), np.load(LOSSES)
    g = fixture_grid(z, name)
    o, d, gt = z[f"{name}_origins"][:N_RESTATED].copy(), z[f"{name}_dirs"][:N_RESTATED].copy(), t[f"{name}_rgb_gt"][:N_RESTATED]
    radius, center = g["radius"], g["center"]
    o[-2], d[-2] = center + 3.0 * radius, np.array([1.0, 0.5, 0.25], np.float32)      # away from the box
    d[-1] = 0.0
    lb, ls = weights(f, name, "both")
    want = GL.fused(g, o, d, gt, beta_loss=lb / N_RESTATED, sparsity_loss=ls, skip=GO.skip_distances(g["links"]), **RESTATED_CASES[case])
    for a in want:
        a.setflags(write=False)
    return o, d, gt, lb, ls, want


@pytest.mark.parametrize("case", sorted(RESTATED_CASES))
@pytest.mark.parametrize("name", ("a", "b", "c"))
def test_volume_render_fused_against_the_restatement(N, name, case):
    """The bar of the existing fused-step test against grid_train_oracle (test_grid_train.assert_matches_restatement): every
    entry within 1e-5 of the tensor's largest. The mask is equal exactly."""
    z = np.load(RENDER)
    g = fixture_grid(z, name)
    o, d, gt, lb, ls, want = restated_case(name, case)
    c = dict(step_size=0.5, sigma_thresh=1e-10, stop_thresh=1e-7, background_brightness=1.0)
    c.update(RESTATED_CASES[case])
    stopped = int((want[4] == np.float32(-1e3)).sum())
    print(f"grid {name} {case}: rays stopped {stopped} of {N_RESTATED}, rows touched {int(want[3].sum())} of {len(want[3])}")
    if case in ("stop", "sigma"):
        assert stopped > 50
    assert want[4][-1] == 0 and want[4][-2] == 0      # the two rays that are not marched
    grid = make_grid(N, g)
    trainer = N.GridTrainer(grid)
    for accelerated in (False, True):
        if accelerated:
            grid.accelerate()
        set_opt(grid, c["background_brightness"], c["step_size"], 0.0, c["sigma_thresh"], c["stop_thresh"])
        label = f"grid {name} {case} {'accelerated' if accelerated else 'plain'}"
        got = run_losses(N, grid, trainer, o, d, gt, lb, ls)
        assert np.array_equal(got[1], want[4]), label      # log_transmit, -1e3 where the ray stopped
        assert assert_matches_restatement(label, got, want[:4]) == 0
        assert np.array_equal(got[4], want[3]), label


# ---- 3. the split route -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("j", (0, 1))
def test_background_trainer_volume_render_fused(N, j):
    z = bg_fixture()
    g = bg_fixture_grid(z)
    nl, step, stop, bright = (float(v) for v in z["settings"][j])
    o, d, gt = z["origins"], z["dirs"], z["rgb_gt"]
    n = o.shape[0]
    grid = TB.setting_grid(N, j, accelerated=True)
    trainer = N.BackgroundTrainer(grid)
    rays = N.Rays(gpu(o), gpu(d))
    keys = ("grad_density", "grad_sh", "grad_background", "mask", "mask_background")

    def state():
        return {k: cpu(getattr(trainer, k)).copy() for k in keys}

    base = TB.run(N, grid, trainer, o, d, gt)      # forward_backward
    # both weights 0: the same to rounding of the sums
    trainer.zero_grad()
    rgb, logt = trainer.volume_render_fused(rays, gpu(gt), return_log_transmit=True)
    assert np.array_equal(cpu(rgb), base["rgb"]) and np.array_equal(cpu(logt), base["log_transmit"])
    off = state()
    for k in keys[:3]:
        noise = float(np.abs(off[k].astype(np.float64) - base[k]).max())
        print(f"setting {j} {k}: weights 0 vs forward_backward max {noise:.3e} (bar {1e-5 * np.abs(base[k]).max():.3e})")
        assert noise <= 1e-5 * np.abs(base[k]).max(), k
    assert np.array_equal(off["mask"], base["mask"]) and np.array_equal(off["mask_background"], base["mask_background"])
    # weights on: grad_density moves by the restatement's loss-only contribution, from the foreground's own log_transmit
    fg = grid.foreground()
    _, logt_fg = fg.volume_render(rays, return_log_transmit=True)
    lb, ls = 1e-3, 8e-6
    kw = dict(step_size=step, sigma_thresh=0.0, stop_thresh=stop)
    terms = GL.loss_terms_density(g, o, d, lb / n, ls, cpu(logt_fg), **kw)
    # the weights suit this grid as the fixture's suit theirs: each term alone is 10 % .. 90 % of the MSE gradient's norm
    alone = [GL.loss_terms_density(g, o, d, one[0] / n, one[1], cpu(logt_fg), **kw) for one in ((lb, 0.0), (0.0, ls))]
    for part in alone:
        share = np.linalg.norm(part) / np.linalg.norm(off["grad_density"])
        assert 0.1 <= share <= 0.9, share
    trainer.zero_grad()
    rgb, logt = trainer.volume_render_fused(rays, gpu(gt), beta_loss=lb, sparsity_loss=ls, return_log_transmit=True)
    assert np.array_equal(cpu(rgb), base["rgb"]) and np.array_equal(cpu(logt), base["log_transmit"])
    on = state()
    moved = on["grad_density"].astype(np.float64) - off["grad_density"]
    big = max(float(np.abs(on["grad_density"]).max()), float(np.abs(off["grad_density"]).max()))
    err = float(np.abs(moved - terms).max())
    worst = int(np.abs(moved - terms).argmax())
    print(f"setting {j}: worst row {worst}: on {on['grad_density'][worst, 0]:.6e} off {off['grad_density'][worst, 0]:.6e} terms {terms[worst, 0]:.6e} "
          f"base {base['grad_density'][worst, 0]:.6e} density {g['density_data'][worst, 0]}")
    print(f"setting {j}: loss terms max {np.abs(terms).max():.3e}, grad_density max {big:.3e}, on - off vs restatement {err:.3e} "
          f"(bar {2e-5 * big + 1.2e-4 * np.abs(alone[0]).max():.3e})")
    # The bar. Each of the two sums is within 1e-5 of its largest entry of its restatement: the bar of the existing tests,
    # twice. And c_beta = beta (1 - T / ((1 - T) + 1e-3)) is ill-conditioned where a ray crosses nearly empty space: at T -> 1 the
    # denominator is 1e-3, so one ulp of T = exp(log_T) (6e-8; the device's expf and numpy's exp are each within one ulp of
    # the exact value, two ulp apart at most) is a relative 2 * 6e-8 / 1e-3 = 1.2e-4 of c_beta, and of the beta term of a row
    # fed by such rays. (On the fixtures of tests 1 and 2 the rays end dark and this is invisible.)
    assert np.abs(terms).max() > 0.05 * big and err <= 2e-5 * big + 1.2e-4 * np.abs(alone[0]).max()
    # the colours, the background and the touched entries do not see the weights
    for k in ("grad_sh", "grad_background"):
        assert np.abs(on[k].astype(np.float64) - off[k]).max() <= 1e-5 * np.abs(off[k]).max(), k
    assert np.array_equal(on["mask"], off["mask"]) and np.array_equal(on["mask_background"], off["mask_background"])


# ---- 4. the recorded loop ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["b", "c"])
def test_train_step_reproduces_the_reference_loop_with_both_terms(N, name):
    z, t, f = np.load(RENDER), np.load(TRAIN), np.load(LOSSES)
    g = fixture_grid(z, name)
    g["density_data"] = (np.float32(0.5) * g["density_data"]).astype(np.float32)
    g["sh_data"] = np.zeros_like(g["sh_data"])
    beta, eps, lr_sh, lr_sigma = f[f"{name}_loop_params"].tolist()
    lb, ls = f[f"{name}_weights"].tolist()
    grid = make_grid(N, g)
    set_opt(grid, 1.0, 0.5, 0.0, 0.0, 0.0)
    grid.accelerate()
    trainer = N.GridTrainer(grid)
    o, d = gpu(z[f"{name}_origins"][:704]), gpu(z[f"{name}_dirs"][:704])
    target = gpu(z[f"{name}_bg1_rgb64"][:704].astype(np.float32))
    losses = []
    for k in t[f"{name}_loop_idx"]:
        k = torch.as_tensor(k.astype(np.int64)).cuda()
        stats = trainer.train_step(N.Rays(o[k], d[k]), target[k], lr_sigma=lr_sigma, lr_sh=lr_sh, beta=beta, epsilon=eps,
                                   lambda_beta=lb, lambda_sparsity=ls)
        losses.append(stats["mse"])
    losses = np.array(losses)
    bars = loop_bars(f, name)
    l64 = f[f"{name}_loop_loss64"]
    dens_err = np.abs(cpu(grid.density_data) - f[f"{name}_loop_density64"]).max()
    sh_err = np.abs(cpu(grid.sh_data) - f[f"{name}_loop_sh64"]).max()
    print(f"grid {name}: loss {losses[0]:.5f} -> {losses[-1]:.5f}; vs fp64 max {np.abs(losses - l64).max():.2e} (bar {bars['loss']:.2e}); "
          f"density {dens_err:.2e} (bar {bars['density']:.2e}); sh {sh_err:.2e} (bar {bars['sh']:.2e})")
    assert np.abs(losses - l64).max() <= bars["loss"]
    assert dens_err <= bars["density"] and sh_err <= bars["sh"]


# ---- 5. the edge rule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRIDS)
def test_tv_gradient_with_the_edge_rule_against_the_restatement(N, name):
    z = np.load(RENDER)
    g = fixture_grid(z, name)
    n = g["links"].size
    cols = g["sh_data"].shape[1]
    grid = make_grid(N, g)
    trainer = N.GridTrainer(grid)
    for target, d0, d1 in (("density", 0, None), ("sh", 0, None), ("sh", 1, cols - 1)):
        trainer.zero_grad()
        start = n - 7      # the range wraps past the last node
        s, count = trainer.add_tv_grad(target, scaling=0.7, sparse_frac=1.0, start=start, start_dim=d0, end_dim=d1, ignore_edge=True)
        assert (s, count) == (start, n)
        table = g["density_data"] if target == "density" else g["sh_data"]
        want, mask = np.zeros_like(table), np.zeros(grid.capacity, np.uint8)
        GL.tv_grad(g, target, start, count, np.float32(0.7) / np.float32(count), want, mask, d0, d1)
        got = cpu(trainer.grad_density if target == "density" else trainer.grad_sh)
        tol = 1e-5 * float(np.abs(want).max())
        err = np.abs(got.astype(np.float64) - want).max()
        print(f"grid {name} tv {target}[{d0}:{d1}] with the edge rule: GPU vs restatement max {err:.3e} (bar {tol:.3e}), rows {int(mask.sum())}")
        assert np.abs(want).max() > 0 and err <= tol
        assert np.array_equal(cpu(trainer.mask), mask)
        assert not cpu(trainer.grad_sh if target == "density" else trainer.grad_density).any()
        if d1 is not None:
            assert not got[:, :d0].any() and not got[:, d1:].any()
        # the rule matters on a sparse grid: far from the gradient without it
        old, mask_old = np.zeros_like(table), np.zeros(grid.capacity, np.uint8)
        GL.tv_grad(g, target, start, count, np.float32(0.7) / np.float32(count), old, mask_old, d0, d1, ignore_edge=False)
        assert np.abs(old - want).max() > 100 * tol


def test_edge_rule_on_the_hand_made_lattice_and_the_flag_off(N):
    def cell(g, xyz, edge):
        grid = make_grid(N, g)
        trainer = N.GridTrainer(grid)
        X, Y, Z = g["links"].shape
        _, count = trainer.add_tv_grad("density", scaling=1.0, sparse_frac=1.5 / 27, start=(xyz[0] * Y + xyz[1]) * Z + xyz[2], ignore_edge=edge)
        assert count == 1
        return cpu(trainer.grad_density).copy(), cpu(trainer.mask).copy()

    check_edge_cases(cell)
    # ignore_edge = 0 through the new entry is the old entry (the same kernel): equal to rounding of the sums
    from nerf_projects_amd import _lib
    z = np.load(RENDER)
    g = fixture_grid(z, "b")
    grid = make_grid(N, g)
    trainer = N.GridTrainer(grid)
    n = g["links"].size
    trainer.add_tv_grad("sh", scaling=0.3, sparse_frac=1.0, start=5)
    old, old_mask = cpu(trainer.grad_sh).copy(), cpu(trainer.mask).copy()
    trainer.zero_grad()
    a = _lib.GridTvArgs()
    a.target, a.start_dim, a.end_dim, a.start, a.count = _lib.NERF_GRID_TV_SH, 0, g["sh_data"].shape[1], 5, n
    a.scale, a.ignore_edge = 0.3 / n, 0
    a.grad, a.mask, a.stream = trainer.grad_sh.data_ptr(), trainer.mask.data_ptr(), trainer.ctx.stream().value
    _lib.check(trainer.ctx.lib.nerf_grid_tv_grad_edge(grid._handle(), C.byref(a)))
    assert old.any() and np.abs(cpu(trainer.grad_sh) - old).max() <= 1e-5 * np.abs(old).max()
    assert np.array_equal(cpu(trainer.mask), old_mask)


# ---- 6. what stays refused, and the new arguments' errors --------------------------------------------------------------
def test_pins_that_stay_and_new_argument_errors(N):
    from nerf_projects_amd import _lib
    z, t = np.load(RENDER), np.load(TRAIN)
    g = fixture_grid(z, "b")
    grid = make_grid(N, g)
    trainer = N.GridTrainer(grid, generator=torch.Generator().manual_seed(3))
    o, d, gt = gpu(z["b_origins"][:64]), gpu(z["b_dirs"][:64]), gpu(t["b_rgb_gt"][:64])
    rays = N.Rays(o, d)
    rgb = trainer.volume_render_fused(rays, gt, beta_loss=0.01, sparsity_loss=1e-6)
    assert torch.equal(rgb, grid.volume_render(rays)) and cpu(trainer.mask).any()
    # in the same process the old names still refuse
    with pytest.raises(NotImplementedError, match="beta_loss.*use volume_render_fused"):
        trainer.forward_backward(rays, gt, beta_loss=0.1)
    with pytest.raises(NotImplementedError, match="sparsity_loss.*use volume_render_fused"):
        trainer.forward_backward(rays, gt, sparsity_loss=0.1)
    lib = trainer.ctx.lib
    tv = _lib.GridTvArgs()
    tv.grad, tv.mask, tv.count, tv.ignore_edge = trainer.grad_density.data_ptr(), trainer.mask.data_ptr(), 1, 1
    assert lib.nerf_grid_tv_grad(grid._handle(), C.byref(tv)) == -1 and b"not built" in lib.nerf_last_error()
    a, opt = _lib.GridFusedArgs(), grid.opt._to_c()
    a.sparsity_loss = 0.5
    assert lib.nerf_grid_fused_backward(grid._handle(), C.byref(opt), C.byref(a)) == -1 and b"sparsity_loss" in lib.nerf_last_error()
    # the new arguments' errors leave the state alone
    before = cpu(trainer.grad_density).copy()
    for kw in (dict(beta_loss=-0.1), dict(sparsity_loss=-1e-3), dict(beta_loss=float("nan")), dict(sparsity_loss=float("inf"))):
        with pytest.raises(ValueError, match="finite and >= 0"):
            trainer.volume_render_fused(rays, gt, **kw)
    with pytest.raises(NotImplementedError, match="randomize"):
        trainer.volume_render_fused(rays, gt, randomize=True)
    grid.opt.last_sample_opaque = True
    with pytest.raises(NotImplementedError, match="last_sample_opaque"):
        trainer.volume_render_fused(rays, gt, beta_loss=0.1)
    grid.opt.last_sample_opaque = False
    assert np.array_equal(cpu(trainer.grad_density), before)
    with pytest.raises(TypeError, match="HalfGrid"):
        N.GridTrainer(grid.to_half())
    # zero rays: nothing happens
    trainer.zero_grad()
    rgb = trainer.volume_render_fused(N.Rays(o[:0], d[:0]), gt[:0], beta_loss=0.1, sparsity_loss=0.1)
    assert rgb.shape == (0, 3) and not cpu(trainer.mask).any()
    # the loop body of the published configurations runs on both trainers: the fused step with both weights, density TV,
    # colour TV with svox2's edge rule, (background TV,) the optimiser steps
    stats = trainer.train_step(rays, gt, lr_sigma=1.0, lambda_tv=1e-4, lambda_tv_sh=1e-3, tv_sparsity=0.05, lambda_beta=1e-5,
                               lambda_sparsity=1e-11, tv_sh_ignore_edge=True)
    assert np.isfinite(stats["mse"])
    zb = bg_fixture()
    bgrid = TB.setting_grid(N, 0, accelerated=True)
    btrainer = N.BackgroundTrainer(bgrid, generator=torch.Generator().manual_seed(4))
    brays, bgt = N.Rays(gpu(zb["origins"][:64]), gpu(zb["dirs"][:64])), gpu(zb["rgb_gt"][:64])
    stats = btrainer.train_step(brays, bgt, lr_sigma=1.0, lambda_tv=1e-4, lambda_tv_sh=1e-3, lambda_tv_background_sigma=1e-3,
                                lambda_tv_background_color=1e-3, tv_sparsity=0.05, tv_background_sparsity=0.05, lambda_beta=1e-5,
                                lambda_sparsity=1e-11, tv_sh_ignore_edge=True)
    assert np.isfinite(stats["mse"]) and cpu(btrainer.mask).any() and cpu(btrainer.mask_background).any()
    with pytest.raises(ValueError, match="ignore_edge"):
        btrainer.add_tv_grad("background", 1.0, ignore_edge=True)
    with pytest.raises(ValueError, match="finite and >= 0"):
        btrainer.volume_render_fused(brays, bgt, beta_loss=-1.0)
    with pytest.raises(NotImplementedError, match="randomize"):
        btrainer.volume_render_fused(brays, bgt, randomize=True)
