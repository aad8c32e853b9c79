"""Training the background layers on the GPU (include/nerf_mi355x.h, "Sparse voxel grid: background layers, training";
nerf-projects_amd/grid_background_train.py): ``BackgroundTrainer`` against the fp64 autograd gradients of
tests/golden/grid_background_train.npz and against the numpy restatement (tests/grid_background_train_oracle.py).
Needs a real MI355X: run with ``pytest -m gpu``.

Bars. Against the golden: ``max(3 d_ref, 1e-5 max |want|)`` per table (``grad_bar``: the reference's own fp32 - fp64 distance).
Against the restatement: 1e-5 of the table's largest entry - kernel and restatement form every term with the same fp32
operations and differ in the order in which at most a few hundred terms are added into an entry (the bar of
tests/test_grid_train.py)."""
import functools

import numpy as np
import pytest
import torch

import grid_background_train_oracle as BT
from test_grid import cpu, gpu, set_opt
from test_grid_background_train_cpu import (N_SETTINGS, TV_SCALES, fixture, fixture_background, fixture_grid, grad_bar,
                                            loop_bars, restated, restated_loop, tv_case)

pytestmark = pytest.mark.gpu

F = np.float32
KEYS = (("density", "grad_density"), ("sh", "grad_sh"), ("background", "grad_background"))


@pytest.fixture(scope="module")
def N():
    import nerf_projects_amd as pkg
    return pkg


def make_grid(N, g, bg):
    return N.BackgroundGrid.from_tensors(gpu(g["links"]), gpu(g["density_data"]), gpu(g["sh_data"]), g["radius"].tolist(),
                                         g["center"].tolist(), background_links=gpu(bg["links"]), background_data=gpu(bg["data"]))


def setting_grid(N, j, accelerated=False, bg=None):
    z = fixture()
    nl, step, stop, bright = z["settings"][j]
    grid = make_grid(N, fixture_grid(z), fixture_background(z, nl) if bg is None else bg)
    set_opt(grid, float(bright), float(step), 0.0, 0.0, float(stop))
    if accelerated:
        grid.accelerate()
    return grid


def run(N, grid, trainer, o, d, gt, zero=True):
    """zero_grad + forward_backward: a dict of numpy arrays; rgb and log_transmit are the renderer's bits"""
    rays = N.Rays(gpu(o), gpu(d))
    if zero:
        trainer.zero_grad()
    rgb, logt = trainer.forward_backward(rays, gpu(gt), return_log_transmit=True)
    want_rgb, want_logt = grid.volume_render(rays, return_log_transmit=True)
    assert torch.equal(rgb, want_rgb) and torch.equal(logt, want_logt)      # bit-identical to the renderer
    out = {k: cpu(getattr(trainer, k)).copy() for k in ("grad_density", "grad_sh", "mask", "grad_background", "mask_background")}
    out.update(rgb=cpu(rgb).copy(), log_transmit=cpu(logt).copy())
    return out


def assert_matches_restatement(label, got, want, factor=1.0):
    """every gradient entry within 1e-5 of the table's largest (times ``factor``); mask_background differing only in rows
    whose restated gradient is below that bar in every entry"""
    for _, key in KEYS:
        w = want[key].astype(np.float64) * factor
        big = float(np.abs(w).max())
        err = float(np.abs(got[key].astype(np.float64) - w).max())
        print(f"{label} {key}: GPU vs restatement max {err:.3e} (bar {1e-5 * big:.3e})")
        assert np.isfinite(got[key]).all() and err <= 1e-5 * big, (label, key, err, big)
    w = want["grad_background"]
    below = (np.abs(w) <= 1e-5 * np.abs(w).max()).all((1, 2))
    differ = ((got["mask_background"] != 0) != (want["mask_background"] != 0)).any(-1)
    assert not (differ & ~below).any(), (label, np.nonzero(differ & ~below)[0][:8])


# ---- 1. every fixture setting ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accelerated", [False, True])
@pytest.mark.parametrize("j", range(N_SETTINGS))
def test_gradients_of_every_fixture_setting(N, j, accelerated):
    z = fixture()
    grid = setting_grid(N, j, accelerated)
    trainer = N.BackgroundTrainer(grid)
    got = run(N, grid, trainer, z["origins"], z["dirs"], z["rgb_gt"])
    bars = {}
    for name, key in KEYS:
        want, tol = grad_bar(z, j, name)
        err = float(np.abs(got[key].astype(np.float64).reshape(want.shape) - want).max())
        print(f"setting {j} {'accelerated' if accelerated else 'plain'} d/d{name}: GPU vs fp64 autograd max {err:.3e} (bar {tol:.3e}, "
              f"max |g| {np.abs(want).max():.3e})")
        assert np.isfinite(got[key]).all() and err <= tol, (name, err, tol)
        bars[key] = tol
    want = restated(j)
    below = (np.abs(want["grad_background"]) <= bars["grad_background"]).all((1, 2))
    differ = ((got["mask_background"] != 0) != (want["mask_background"] != 0)).any(-1)
    assert not (differ & ~below).any() and got["mask_background"].any()
    assert not got["grad_background"][got["mask_background"] == 0].any()
    # a second call accumulates
    twice = run(N, grid, trainer, z["origins"], z["dirs"], z["rgb_gt"], zero=False)
    for _, key in KEYS:
        err = float(np.abs(twice[key].astype(np.float64) - 2.0 * got[key]).max())
        assert err <= 2.0 * bars[key], (key, err)


# ---- 2. the foreground's gradients are complete ------------------------------------------------------------------------
def test_foreground_gradients_contain_the_background_term(N):
    z = fixture()
    j = 4
    grid = setting_grid(N, j)
    got = run(N, grid, N.BackgroundTrainer(grid), z["origins"], z["dirs"], z["rgb_gt"])
    fg = grid.foreground()
    alone = N.GridTrainer(fg)
    alone.zero_grad()
    alone.forward_backward(N.Rays(gpu(z["origins"]), gpu(z["dirs"])), gpu(z["rgb_gt"]))
    _, tol = grad_bar(z, j, "density")
    diff = float(np.abs(got["grad_density"] - cpu(alone.grad_density)).max())
    print(f"density gradient with and without what lies behind the samples: {diff:.3e} apart (bar {tol:.3e})")
    assert diff > 100 * tol      # today's composition (a foreground trained next to a frozen background) is another gradient
    # a background without positive sigma adds exp(log_T) * brightness only: the foreground-only trainer's gradients
    bg = fixture_background(z, z["settings"][j][0])
    dark = {"links": bg["links"], "data": bg["data"].copy()}
    dark["data"][..., 3] = -np.abs(dark["data"][..., 3])
    grid2 = setting_grid(N, j, bg=dark)
    got2 = run(N, grid2, N.BackgroundTrainer(grid2), z["origins"], z["dirs"], z["rgb_gt"])
    for name, key in KEYS[:2]:
        _, tol = grad_bar(z, j, name)
        err = float(np.abs(got2[key] - cpu(getattr(alone, key))).max())
        print(f"no positive sigma, d/d{name}: {err:.3e} from the foreground-only trainer (bar {tol:.3e})")
        assert err <= tol
    assert not got2["grad_background"].any() and not got2["mask_background"].any()


# ---- 3. batch edges ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_rays():
    """257 finite fixture rays that reach the layers, a third of them through the box"""
    z = fixture()
    r = restated(5)
    ok = z["setup_ok"] & ~(r["fg_log_transmit"] < -25)
    return np.nonzero(ok)[0][:257]


@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 9, 63, 64, 65, 255, 256, 257])
def test_batches_around_a_wavefront_and_a_workgroup(N, n):
    """the shipped backward gives a ray 32 lanes: 2 rays per wavefront, 8 per workgroup; the taped pass 64 and 256"""
    z = fixture()
    j = 5
    nl, step, stop, bright = z["settings"][j]
    k = edge_rays()[:n]
    o, d, gt = z["origins"][k], z["dirs"][k], z["rgb_gt"][k]
    grid = setting_grid(N, j)
    got = run(N, grid, N.BackgroundTrainer(grid), o, d, gt)
    want = BT.forward_backward(fixture_grid(z), fixture_background(z, nl), o, d, gt, float(step), 0.0, float(stop), float(bright))
    assert np.array_equal(got["rgb"], want["rgb"]) or np.abs(got["rgb"] - want["rgb"]).max() <= 1e-5
    assert_matches_restatement(f"{n} rays", got, want)


def test_a_batch_is_the_sum_of_its_halves(N):
    """257 rays against their two halves run alone, each scaled by n_half / n (the loss is a mean)"""
    z = fixture()
    k = edge_rays()
    n, h = len(k), len(k) // 2
    grid = setting_grid(N, 5)
    trainer = N.BackgroundTrainer(grid)
    part = [run(N, grid, trainer, z["origins"][s], z["dirs"][s], z["rgb_gt"][s]) for s in (k, k[:h], k[h:])]
    assert np.array_equal(part[0]["rgb"], np.concatenate([part[1]["rgb"], part[2]["rgb"]]))
    assert np.array_equal(part[0]["mask_background"], part[1]["mask_background"] | part[2]["mask_background"])
    for _, key in KEYS:
        want = part[1][key].astype(np.float64) * (h / n) + part[2][key].astype(np.float64) * ((n - h) / n)
        err, big = float(np.abs(part[0][key] - want).max()), float(np.abs(want).max())
        print(f"{n} rays vs {h} + {n - h}, {key}: {err:.3e} = {err / big:.2e} of the largest entry")
        assert big > 0 and err <= 1e-5 * big


# ---- 4. contention, hostile and left-alone rays ------------------------------------------------------------------------
def test_two_thousand_copies_of_one_ray(N):
    """2 000 copies of a ray that crosses the foreground and the layers: every term is added 2 000 times into the same
    entries. The MSE's factor is 1 / n, so the batch's gradient is 2 000 x (the single ray's / 2 000): the single ray's. The bar
    against the single ray is 2 000 x 2^-24 = 1.2e-4 of the largest entry, the bound on 2 000 fp32 additions into one running
    sum (each rounds to half an ulp of the sum). The restatement of the same batch adds the same terms in another order and is
    as far from the exact sum, so the bar against it is twice that, 2.4e-4 - an add lost to a race costs 1 / 2 000 = 5e-4 of its
    entry. (Measured on the MI355X: at most 6.7e-5 from the single ray, 1.2e-4 from the restatement.)"""
    z = fixture()
    j = 5
    nl, step, stop, bright = z["settings"][j]
    r = restated(j)
    through = z["setup_ok"] & (r["fg_log_transmit"] > -2.5) & (r["fg_log_transmit"] < -0.2)
    k = int(np.argmax(np.abs(r["grad_rgb"]).sum(-1) * through))
    bar = 2000 * 2.0 ** -24
    one = (z["origins"][k:k + 1], z["dirs"][k:k + 1], z["rgb_gt"][k:k + 1])
    many = tuple(np.repeat(a, 2000, 0) for a in one)
    grid = setting_grid(N, j)
    trainer = N.BackgroundTrainer(grid)
    a = run(N, grid, trainer, *one)
    b = run(N, grid, trainer, *many)
    want = BT.forward_backward(fixture_grid(z), fixture_background(z, nl), *many, float(step), 0.0, float(stop), float(bright))
    assert np.array_equal(a["mask_background"], b["mask_background"]) and a["mask_background"].sum() >= 8
    assert np.array_equal(b["mask_background"] != 0, want["mask_background"] != 0)
    for _, key in KEYS:
        big = float(np.abs(a[key]).max())
        assert big > 0, key
        err = float(np.abs(b[key].astype(np.float64) - a[key]).max())
        err_r = float(np.abs(b[key].astype(np.float64) - want[key]).max())
        print(f"{key}: 2000 copies vs the single ray {err / big:.2e}, vs the restatement {err_r / big:.2e} of the largest entry "
              f"(bars {bar:.2e}, {2 * bar:.2e})")
        assert np.isfinite(b[key]).all() and err <= bar * big and err_r <= 2.0 * bar * big


def test_hostile_and_left_alone_rays_give_no_gradient(N):
    z = fixture()
    j = 3
    r = restated(j)
    grid = setting_grid(N, j)
    trainer = N.BackgroundTrainer(grid)
    hostile = np.nonzero(~z["setup_ok"])[0]
    dark = np.nonzero(z["setup_ok"] & (r["fg_log_transmit"] < -25))[0]
    assert len(hostile) >= 16 and len(dark) >= 16
    zero_dir = (z["dirs"][hostile] == 0).all(-1)
    assert zero_dir.any() and np.isnan(z["origins"][hostile]).any() and np.isinf(z["dirs"][hostile]).any()
    got = run(N, grid, trainer, z["origins"][hostile], z["dirs"][hostile], z["rgb_gt"][hostile])
    assert not got["grad_background"].any() and not got["mask_background"].any()
    assert not got["grad_density"].any() and not got["grad_sh"].any()
    got = run(N, grid, trainer, z["origins"][dark], z["dirs"][dark], z["rgb_gt"][dark])
    assert not got["grad_background"].any() and not got["mask_background"].any()      # left alone: nothing added
    assert got["grad_density"].any()                                                     # (the foreground did train)
    # inside a batch they change nothing but the mean's factor, and every table stays finite
    good = np.nonzero(z["setup_ok"] & ~(r["fg_log_transmit"] < -25))[0][:100]
    mixed = np.concatenate([hostile[:8], good, dark[:8], hostile[8:]])
    a = run(N, grid, trainer, z["origins"][good], z["dirs"][good], z["rgb_gt"][good])
    b = run(N, grid, trainer, z["origins"][mixed], z["dirs"][mixed], z["rgb_gt"][mixed])
    assert all(np.isfinite(b[key]).all() for _, key in KEYS)
    want = a["grad_background"].astype(np.float64) * (len(good) / len(mixed))
    assert np.abs(b["grad_background"] - want).max() <= 1e-5 * np.abs(want).max()
    assert np.array_equal(a["mask_background"], b["mask_background"])


def test_rows_past_two_gib(N):
    """capacity * L * 16 bytes just past 2^31, only the last rows linked: the gradient lands there, the rows below stay zero"""
    z = fixture()
    R, L = 8, 64
    texels = 2 * R * R
    cap = (1 << 31) // (L * 16) + texels
    rng = np.random.default_rng(5)
    data = torch.zeros((cap, L, 4), dtype=torch.float32, device="cuda")
    last = rng.normal(0.0, 1.0, (texels, L, 4)).astype(F)
    last[..., 3] = rng.uniform(0.0, 2.0, (texels, L))
    data[cap - texels:] = gpu(last)
    links = gpu((cap - texels + rng.permutation(texels)).astype(np.int32).reshape(2 * R, R))
    g = fixture_grid(z)
    grid = N.BackgroundGrid.from_tensors(gpu(g["links"]), gpu(g["density_data"]), gpu(g["sh_data"]), g["radius"].tolist(),
                                         g["center"].tolist(), background_links=links, background_data=data)
    set_opt(grid, 1.0, 0.5, 0.0, 0.0, 1e-7)
    trainer = N.BackgroundTrainer(grid)
    k = edge_rays()[:64]
    rays = N.Rays(gpu(z["origins"][k]), gpu(z["dirs"][k]))
    rgb = trainer.forward_backward(rays, gpu(z["rgb_gt"][k]))
    assert torch.equal(rgb, grid.volume_render(rays))
    gb, mb = trainer.grad_background, trainer.mask_background
    assert gb.numel() * 4 > 1 << 31
    assert not bool(gb[:cap - texels].any()) and not bool(mb[:cap - texels].any())
    tail = cpu(gb[cap - texels:])
    assert np.isfinite(tail).all() and (tail != 0).any((1, 2)).sum() >= texels // 4
    # the small table with the same rows gives the same gradient
    small = N.BackgroundGrid.from_tensors(gpu(g["links"]), gpu(g["density_data"]), gpu(g["sh_data"]), g["radius"].tolist(),
                                          g["center"].tolist(), background_links=links - (cap - texels), background_data=gpu(last))
    set_opt(small, 1.0, 0.5, 0.0, 0.0, 1e-7)
    t2 = N.BackgroundTrainer(small)
    t2.forward_backward(rays, gpu(z["rgb_gt"][k]))
    want = cpu(t2.grad_background)
    assert np.abs(tail - want).max() <= 1e-5 * np.abs(want).max()
    assert np.array_equal(cpu(mb[cap - texels:]), cpu(t2.mask_background))
    # the step reaches them too
    before = data[cap - texels:].clone()
    trainer.step(0.0, 0.0, 0.1, 0.1)
    assert not torch.equal(before, data[cap - texels:]) and not bool(data[:cap - texels].any())


# ---- 5. TV and the optimiser -------------------------------------------------------------------------------------------
def test_tv_and_optimiser_match_their_restatements(N):
    z = fixture()
    bg, cells, want64, want, want_mask = tv_case()
    grid = make_grid(N, fixture_grid(z), bg)
    trainer = N.BackgroundTrainer(grid)
    start, count = trainer.add_tv_grad("background", TV_SCALES[1], TV_SCALES[0], sparse_frac=1.0, start=cells - 7)
    assert (start, count) == (cells - 7, cells)
    got = cpu(trainer.grad_background)
    for sl in (slice(0, 3), slice(3, 4)):
        big = float(np.abs(want[..., sl]).max())
        err = float(np.abs(got[..., sl] - want[..., sl]).max())
        err64 = float(np.abs(got[..., sl] - want64[..., sl]).max())
        print(f"tv channels {sl}: GPU vs restatement {err:.3e}, vs fp64 autograd {err64:.3e} (bar {1e-5 * big:.3e})")
        assert err <= 1e-5 * big and err64 <= 1e-5 * big
    assert np.array_equal(cpu(trainer.mask_background), want_mask)
    assert not cpu(trainer.grad_density).any() and not cpu(trainer.mask).any()
    s2, c2 = trainer.add_tv_grad("background", 1.0, sparse_frac=0.1)      # the start comes from the generator
    assert c2 == max(1, int(0.1 * cells)) and 0 <= s2 < cells
    assert trainer.add_tv_grad("density", 1.0, sparse_frac=0.5)[1] == max(1, int(0.5 * grid.links.numel()))
    # the optimiser, bit for bit: a masked-off entry, a NaN gradient, an rms of zero, both kinds
    rng = np.random.default_rng(3)
    shape = tuple(bg["data"].shape)
    for kind in ("rmsprop", "sgd"):
        data = bg["data"].copy()
        rms = ((rng.random(shape) < 0.5) * rng.random(shape)).astype(F)
        grad = rng.normal(0.0, 1e-2, shape).astype(F)
        grad[1, 1, 2], grad[2, 0, 3], grad[3, 2, 0] = np.nan, np.inf, F(1e-30)
        mask = (rng.random(shape[:2]) < 0.7).astype(np.uint8)
        mask[0, 0], mask[1, 1] = 0, 5
        trainer.zero_grad()      # (the foreground's mask is empty: its tables do not move)
        grid.background_data.copy_(gpu(data))
        trainer.background_rms.copy_(gpu(rms))
        trainer.grad_background.copy_(gpu(grad))
        trainer.mask_background.copy_(gpu(mask))
        dens = grid.density_data.clone()
        trainer.step(1.0, 1.0, 0.5, 1e-2, optim=kind)
        BT.optim_step(data, rms, grad, mask, kind, 0.5, 1e-2)
        assert np.array_equal(cpu(grid.background_data), data, equal_nan=True), kind
        assert np.array_equal(cpu(trainer.background_rms), rms, equal_nan=True), kind
        assert torch.equal(dens, grid.density_data)
        assert data[1, 1, 2] == F(-1e9)


# ---- 6. a training loop ------------------------------------------------------------------------------------------------
def test_train_step_loop_follows_the_restatement(N):
    z = fixture()
    bars = loop_bars(z)
    want = restated_loop()
    j = int(want["setting"])
    nl, step, stop, bright = z["settings"][j]
    beta, eps, lr_sh, lr_sigma, lr_sigma_bg, lr_color_bg = z["loop_params"]
    g = dict(fixture_grid(z), density_data=want["density0"], sh_data=want["sh0"])
    grid = make_grid(N, g, {"links": fixture_background(z, nl)["links"], "data": want["background0"]})
    set_opt(grid, float(bright), float(step), 0.0, 0.0, float(stop))
    grid.accelerate()
    trainer = N.BackgroundTrainer(grid)
    target = z[f"set{j}_rgb64"].astype(F)
    losses = []
    for k in z["loop_idx"]:
        out = trainer.train_step(N.Rays(gpu(z["origins"][k]), gpu(z["dirs"][k])), gpu(target[k]), lr_sigma=float(lr_sigma),
                                 lr_sh=float(lr_sh), lr_sigma_bg=float(lr_sigma_bg), lr_color_bg=float(lr_color_bg), beta=float(beta),
                                 epsilon=float(eps))
        losses.append(out["mse"])
    err = float(np.abs(np.array(losses) - want["loss"]).max())
    print(f"loop loss {losses[0]:.5f} -> {losses[-1]:.5f}: GPU vs restatement {err:.3e} (bar {bars['loss']:.3e})")
    assert losses[-1] < 0.5 * losses[0] and err <= bars["loss"]
    for key, t in (("density", grid.density_data), ("sh", grid.sh_data), ("background", grid.background_data)):
        e = float(np.abs(cpu(t).astype(np.float64) - want[key]).max())
        print(f"loop final {key}: GPU vs restatement {e:.3e} (bar {bars[key]:.3e})")
        assert e <= bars[key], key


# ---- 7. state and errors -----------------------------------------------------------------------------------------------
def test_state_across_renders_shape_changes_and_errors(N):
    z = fixture()
    j = 2
    grid = setting_grid(N, j, accelerated=True)
    trainer = N.BackgroundTrainer(grid)
    k = edge_rays()[:128]
    rays, gt = N.Rays(gpu(z["origins"][k]), gpu(z["dirs"][k])), gpu(z["rgb_gt"][k])
    before = grid.volume_render(rays)
    h = grid._handle()
    trainer.train_step(rays, gt, lr_sigma=1.0, lr_sh=1e-2, lr_sigma_bg=0.5, lr_color_bg=1e-2, lambda_tv_background_sigma=1e-3,
                       lambda_tv_background_color=1e-3, tv_background_sparsity=0.5)
    assert grid._handle() == h and grid.accelerated      # no new handle, the skip data survives
    assert not torch.equal(before, grid.volume_render(rays))      # renders see the trained values
    assert bool(trainer.background_rms.any()) and bool(trainer.density_rms.any())
    # argument errors leave the trainer usable
    with pytest.raises(ValueError):
        trainer.forward_backward(rays, gt[:5])
    with pytest.raises(RuntimeError):
        trainer.forward_backward(rays, gt.cpu())
    with pytest.raises(ValueError):
        trainer.add_tv_grad("layers")
    with pytest.raises(ValueError):
        trainer.add_tv_grad("background", 1.0, start=10 ** 9)
    with pytest.raises(ValueError):
        trainer.step(1.0, 1.0, 1.0, 1.0, optim="adam")
    with pytest.raises(ValueError):
        trainer.sparsify_background(float("nan"))
    with pytest.raises(TypeError):
        N.BackgroundTrainer(grid.foreground())
    trainer.zero_grad()
    assert not any(bool(getattr(trainer, a).any()) for a in ("grad_density", "grad_sh", "mask", "grad_background", "mask_background"))
    trainer.train_step(rays, gt)
    # sparsify_background: the background's state anew, the foreground's kept
    rms_d = trainer.density_rms.clone()
    kept = trainer.sparsify_background(1.0, 1)
    assert kept == grid.background_data.shape[0] and tuple(trainer.grad_background.shape) == tuple(grid.background_data.shape)
    assert not bool(trainer.background_rms.any()) and torch.equal(rms_d, trainer.density_rms) and grid.accelerated
    trainer.train_step(rays, gt)
    # resample / remove_floaters: the foreground's state anew, the background's kept
    rms_b = trainer.background_rms.clone()
    assert bool(rms_b.any())
    trainer.resample((10, 12, 8), sigma_thresh=0.0, weight_thresh=0.0, dilate=1)
    assert tuple(grid.links.shape) == (10, 12, 8) and tuple(trainer.grad_density.shape) == tuple(grid.density_data.shape)
    assert not bool(trainer.density_rms.any()) and torch.equal(rms_b, trainer.background_rms) and grid.accelerated
    trainer.train_step(rays, gt)
    rms_b = trainer.background_rms.clone()
    assert bool(trainer.density_rms.any())
    trainer.remove_floaters(min_object_size=1, use_adaptive=False)
    assert tuple(trainer.grad_sh.shape) == tuple(grid.sh_data.shape) and torch.equal(rms_b, trainer.background_rms)
    assert not bool(trainer.density_rms.any()) and grid.accelerated
    out = trainer.train_step(rays, gt)
    assert np.isfinite(out["mse"])
    with pytest.raises((ValueError, RuntimeError)):
        trainer.resample((1, 2, 3))
    trainer.train_step(rays, gt)
    # a background_data of another shape is an error at the next call
    grid.background_data = torch.cat([grid.background_data, grid.background_data[:1]])
    with pytest.raises(ValueError, match="changed shape"):
        trainer.forward_backward(rays, gt)
    # the refusals of the foreground-only classes stay
    with pytest.raises(NotImplementedError, match="foreground"):
        N.GridTrainer(grid)
