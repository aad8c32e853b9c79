"""``loss.backward()`` through the sparse voxel grid on the GPU (include/nerf_mi355x.h, "Sparse voxel grid: gradients for
autograd"): ``GridModule`` against the reference's recorded gradients (tests/golden/grid_autograd.npz), against the numpy
restatement (tests/grid_autograd_oracle.py, checked against the same fixture in tests/test_grid_autograd_cpu.py), and
against ``GridTrainer.forward_backward``; batch edges, hostile rays, hand-made sample points, the module's contract and an
Adam loop. Needs a real MI355X: run with ``pytest -m gpu``."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import grid_autograd_oracle as GA
import grid_oracle as GO
from test_grid import cpu, gpu, make_grid, random_grid, random_grid_with_faces, set_opt
from test_grid_autograd_cpu import AUTOGRAD, BACKGROUNDS, GRIDS, RENDER, TRAIN, fixture_grid, grad_bar
from test_grid_train import LANES, THRESHOLD_CASES, hostile_rays, mixed_rays, through_rays
from test_grid_train_cpu import grad_bar as train_grad_bar

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def N():
    import nerf_projects_amd as pkg
    return pkg


def fixture_camera(N, z):
    fx, fy, cx, cy = z["cam_intrinsics"].tolist()
    w, h = (int(v) for v in z["cam_size"])
    return N.Camera(torch.from_numpy(z["cam_c2w"]), fx=fx, fy=fy, cx=cx, cy=cy, width=w, height=h)


def vjp(m, o, d, cot):
    """(rgb, grad_density, grad_sh) of ``m.volume_render`` with the cotangent ``cot`` (numpy in, numpy out)"""
    from nerf_projects_amd import Rays
    m.zero_grad(set_to_none=True)
    rgb = m.volume_render(Rays(gpu(o), gpu(d)))
    rgb.backward(gpu(np.asarray(cot, np.float32)))
    return cpu(rgb).copy(), cpu(m.density_data.grad).copy(), cpu(m.sh_data.grad).copy()


def c_backward(N, grid, o, d, cot, tables=(True, True, True)):
    """The two C calls themselves, mask included: (rgb, grad_density, grad_sh, mask) as numpy, None where not asked for"""
    from nerf_projects_amd import _lib
    o_t, d_t, cot_t = gpu(o), gpu(d), gpu(np.asarray(cot, np.float32))
    n, cap, cols = o_t.shape[0], grid.capacity, grid.sh_data.shape[1]
    dev = o_t.device
    rgb = torch.empty((n, 3), device=dev)
    tape = torch.empty((n, 3), device=dev, dtype=torch.float64)
    opt = grid.opt._to_c()
    a = _lib.GridRenderTapedArgs()
    a.origins, a.dirs, a.n_rays, a.rgb_out, a.tape = o_t.data_ptr(), d_t.data_ptr(), n, rgb.data_ptr(), tape.data_ptr()
    a.use_skip, a.stream = 1, grid.ctx.stream().value
    _lib.check(grid.ctx.lib.nerf_grid_render_rays_taped(grid._handle(), C.byref(opt), C.byref(a)))
    gd = torch.zeros((cap, 1), device=dev) if tables[0] else None
    gs = torch.zeros((cap, cols), device=dev) if tables[1] else None
    mask = torch.zeros((cap,), device=dev, dtype=torch.uint8) if tables[2] else None
    b = _lib.GridRenderBackwardArgs()
    b.origins, b.dirs, b.n_rays, b.grad_rgb, b.tape = o_t.data_ptr(), d_t.data_ptr(), n, cot_t.data_ptr(), tape.data_ptr()
    b.grad_density, b.grad_sh, b.mask = (0 if t is None else t.data_ptr() for t in (gd, gs, mask))
    b.use_skip, b.stream = 1, grid.ctx.stream().value
    _lib.check(grid.ctx.lib.nerf_grid_render_backward(grid._handle(), C.byref(opt), C.byref(b)))
    return (cpu(rgb).copy(),) + tuple(None if t is None else cpu(t).copy() for t in (gd, gs, mask))


def assert_close(label, got, want, rel=1e-5):
    """every entry within ``rel`` of the tensor's largest"""
    big = float(np.abs(want).max())
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{label}: max {err:.3e} = {err / big if big else 0.0:.2e} of the largest entry (bar {rel * big:.3e})")
    assert np.isfinite(got).all() and big > 0 and err <= rel * big, (label, err, rel * big)


# ---- 1. the forward is the renderer and the sampler, bit for bit --------------------------------------------------------
@pytest.mark.parametrize("name", ("a", "b", "c"))      # basis_dim 9, 4, 1
def test_forward_is_bit_identical_with_and_without_grad(N, name):
    z = np.load(RENDER)
    grid = make_grid(N, fixture_grid(z, name))
    m = N.GridModule(grid)
    rays = N.Rays(gpu(z[f"{name}_origins"]), gpu(z[f"{name}_dirs"]))
    cam = fixture_camera(N, z)
    pts = gpu(z[f"{name}_pts_world"])
    for accelerated in (False, True):
        if accelerated:
            grid.accelerate()
        assert grid.accelerated == accelerated
        want_rgb, want_img, want_s = grid.volume_render(rays), grid.volume_render_image(cam), grid.sample(pts)
        want_d0, want_s0 = grid.sample(pts, want_colors=False)
        for grad in (True, False):
            with torch.set_grad_enabled(grad):
                rgb, img, (dens, sh) = m.volume_render(rays), m.volume_render_image(cam), m.sample(pts)
                d0, s0 = m.sample(pts, want_colors=False)
            assert rgb.requires_grad == grad and img.requires_grad == grad and dens.requires_grad == grad
            assert torch.equal(rgb, want_rgb) and torch.equal(img, want_img) and img.shape == want_img.shape
            assert torch.equal(dens, want_s[0]) and torch.equal(sh, want_s[1])
            assert torch.equal(d0, want_d0) and s0.shape == want_s0.shape and not s0.requires_grad
    pg = gpu(z[f"{name}_pts_grid"])
    assert all(torch.equal(x, y) for x, y in zip(m.sample(pg, grid_coords=True), grid.sample(pg, grid_coords=True)))


# ---- 2. the reference's gradients ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRIDS)
def test_render_backward_against_the_reference_autograd(N, name):
    """Golden (i), the vector-Jacobian product with a recorded cotangent, and (ii), a Charbonnier loss through torch's own
    autograd, at both backgrounds, plain and accelerated: every entry within max(3 d_ref, 1e-5 max |g64|)."""
    z, t, a = np.load(RENDER), np.load(TRAIN), np.load(AUTOGRAD)
    grid = make_grid(N, fixture_grid(z, name))
    m = N.GridModule(grid)
    rays = N.Rays(gpu(z[f"{name}_origins"]), gpu(z[f"{name}_dirs"]))
    w, gt, eps = gpu(a[f"{name}_vjp_w"]), gpu(t[f"{name}_rgb_gt"]), float(a["charb_eps"])
    losses = {"vjp": lambda rgb: (rgb * w).sum(), "charb": lambda rgb: torch.sqrt((rgb - gt) ** 2 + eps).mean()}
    for accelerated in (False, True):
        if accelerated:
            grid.accelerate()
        for tag, bg in BACKGROUNDS:
            set_opt(grid, bg, 0.5, 0.0, 0.0, 0.0)
            for kind, loss_of in losses.items():
                m.zero_grad(set_to_none=True)
                rgb = m.volume_render(rays)
                assert torch.equal(rgb, grid.volume_render(rays))
                loss_of(rgb).backward()
                for key, got in (("density", m.density_data.grad), ("sh", m.sh_data.grad)):
                    want, tol = grad_bar(a, name, tag, kind, key)
                    err = np.abs(cpu(got).astype(np.float64) - want)
                    print(f"grid {name} {tag} {kind} {'accelerated' if accelerated else 'plain'} d/d{key}: GPU vs fp64 autograd "
                          f"max {err.max():.3e} (bar {tol:.3e}, max |g| {np.abs(want).max():.3e})")
                    assert got.shape == want.shape and np.isfinite(cpu(got)).all()
                    assert err.max() <= tol, (name, tag, kind, key, int(err.argmax()), err.max(), tol)      # every entry


# ---- 3. off-default options on grids that keep their faces, against the restatement -----------------------------------
@pytest.mark.parametrize("case", sorted(THRESHOLD_CASES))
@pytest.mark.parametrize("basis_dim,reso", [(9, (28, 30, 32)), (4, (29, 31, 30)), (1, (32, 30, 28))])
def test_render_backward_off_default_options_with_kept_faces(N, basis_dim, reso, case):
    rng = np.random.default_rng(700 + basis_dim)
    g = random_grid_with_faces(rng, reso, basis_dim, keep=0.3, sh_std=4.0)
    assert all((f >= 0).any() for f in (g["links"][0], g["links"][-1], g["links"][:, 0], g["links"][:, -1], g["links"][:, :, 0],
                                        g["links"][:, :, -1]))
    o, d = mixed_rays(rng, g, 600)
    cot = rng.normal(size=(600, 3)).astype(np.float32)
    c = THRESHOLD_CASES[case]
    skip = GO.skip_distances(g["links"])
    rgb_o, gd_o, gs_o, mask_o = GA.render_vjp(g, o, d, cot, skip=skip, **c)
    grid = make_grid(N, g)
    m = N.GridModule(grid)
    for accelerated in (False, True):
        if accelerated:
            grid.accelerate()
        set_opt(grid, c["background_brightness"], c["step_size"], c["near_clip"], c["sigma_thresh"], c["stop_thresh"])
        label = f"B = {basis_dim} {case} {'accelerated' if accelerated else 'plain'}"
        rgb, gd, gs = vjp(m, o, d, cot)
        assert np.abs(rgb - rgb_o).max() <= 1e-5
        assert_close(label + " d/ddensity", gd, gd_o)
        assert_close(label + " d/dsh", gs, gs_o)


# ---- 4. the fused kernel's own cotangent ------------------------------------------------------------------------------
def test_mse_cotangent_agrees_with_forward_backward(N):
    """With g = (rgb - gt) * (2 / (3 N)), the fused kernel's own, the backward adds the very same terms; only the order in
    which the atomics arrive differs. The mask is equal; the gradients are within the bar two identical fused calls are held to."""
    z, t = np.load(RENDER), np.load(TRAIN)
    grid = make_grid(N, fixture_grid(z, "a"))
    set_opt(grid, 1.0, 0.5, 0.0, 0.0, 0.0)
    trainer = N.GridTrainer(grid)
    o, d = z["a_origins"], z["a_dirs"]
    rays, gt = N.Rays(gpu(o), gpu(d)), gpu(t["a_rgb_gt"])
    for accelerated in (False, True):
        if accelerated:
            grid.accelerate()
        trainer.zero_grad()
        rgb = trainer.forward_backward(rays, gt)
        scale = torch.tensor(2.0) / (torch.tensor(3.0) * torch.tensor(float(o.shape[0])))      # the kernel's fp32 operations
        cot = cpu((rgb - gt) * scale.to(rgb.device))
        rgb2, gd, gs, mask = c_backward(N, grid, o, d, cot)
        assert np.array_equal(rgb2, cpu(rgb)) and np.array_equal(mask, cpu(trainer.mask)) and mask.any()
        for key, got, fused in (("density", gd, trainer.grad_density), ("sh", gs, trainer.grad_sh)):
            _, tol = train_grad_bar(t, "a", "bg1", key)
            diff = float(np.abs(got.astype(np.float64) - cpu(fused)).max())
            print(f"{'accelerated' if accelerated else 'plain'} d/d{key}: backward vs forward_backward {diff:.3e} = "
                  f"{diff / np.abs(cpu(fused)).max():.2e} of the largest entry (bar {tol:.3e})")
            assert diff <= tol
        # the module delivers the same through autograd
        m = N.GridModule(grid)
        out = m.volume_render(rays)
        ((out - gt) ** 2).mean().backward()
        for key, got, fused in (("density", m.density_data.grad, trainer.grad_density), ("sh", m.sh_data.grad, trainer.grad_sh)):
            _, tol = train_grad_bar(t, "a", "bg1", key)
            assert float((got - fused).abs().max()) <= tol, key


# ---- 5. sample backward -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRIDS)
def test_sample_backward_against_the_reference_autograd(N, name):
    z, a = np.load(RENDER), np.load(AUTOGRAD)
    grid = make_grid(N, fixture_grid(z, name))
    m = N.GridModule(grid)
    cd, cs = gpu(a[f"{name}_sample_cd"]), gpu(a[f"{name}_sample_cs"])
    dens, sh = m.sample(gpu(z[f"{name}_pts_grid"]), grid_coords=True)
    ((dens * cd).sum() + (sh * cs).sum()).backward()
    for key, got in (("density", m.density_data.grad), ("sh", m.sh_data.grad)):
        want, tol = grad_bar(a, name, "", "sample", key)
        err = np.abs(cpu(got).astype(np.float64) - want)
        print(f"grid {name} sample d/d{key}: GPU vs fp64 autograd max {err.max():.3e} (bar {tol:.3e}), rows != 0 {int((want != 0).any(-1).sum())}")
        assert err.max() <= tol, (name, key, int(err.argmax()), err.max(), tol)
    # world coordinates against the restatement
    g = fixture_grid(z, name)
    m.zero_grad(set_to_none=True)
    dens, sh = m.sample(gpu(z[f"{name}_pts_world"]))
    ((dens * cd).sum() + (sh * cs).sum()).backward()
    gd_o, gs_o = GA.sample_backward(g, z[f"{name}_pts_world"], a[f"{name}_sample_cd"], a[f"{name}_sample_cs"])
    for got, want in ((m.density_data.grad, gd_o), (m.sh_data.grad, gs_o)):
        assert np.abs(cpu(got).astype(np.float64) - want).max() <= 1e-5 * max(float(np.abs(want).max()), 1e-30)


def hand_grid(basis_dim=4):
    """6 x 5 x 7, every node kept but the 8 corners of cell (0, 0, 0); rows in random order"""
    rng = np.random.default_rng(11)
    reso = (6, 5, 7)
    kept = np.ones(reso, dtype=bool)
    kept[:2, :2, :2] = False
    n = int(kept.sum())
    links = np.full(reso, -1, dtype=np.int32)
    links[kept] = rng.permutation(n).astype(np.int32)
    return {"links": links, "density_data": rng.uniform(0, 5, (n, 1)).astype(np.float32),
            "sh_data": rng.normal(size=(n, 3 * basis_dim)).astype(np.float32), "radius": np.array([1.0, 1.2, 0.9], np.float32),
            "center": np.array([0.1, 0.0, -0.1], np.float32)}


def sample_grads(m, pts, go_d, go_s, want_colors=True):
    m.zero_grad(set_to_none=True)
    dens, sh = m.sample(gpu(np.asarray(pts, np.float32)), grid_coords=True, want_colors=want_colors)
    loss = (dens * gpu(go_d)).sum()
    if want_colors:
        loss = loss + (sh * gpu(go_s)).sum()
    loss.backward()
    return cpu(m.density_data.grad).copy(), None if m.sh_data.grad is None else cpu(m.sh_data.grad).copy()


def test_sample_backward_at_hand_made_points(N):
    g = hand_grid()
    links = g["links"]
    grid = make_grid(N, g)
    m = N.GridModule(grid)
    rng = np.random.default_rng(12)
    go_d = (np.round(rng.normal(size=(1, 1)) * 16) / 16 + 0.0625).astype(np.float32)
    go_s = (np.round(rng.normal(size=(1, 12)) * 16) / 16 + 0.0625).astype(np.float32)

    def one_row(pt, row):
        gd, gs = sample_grads(m, [pt], go_d, go_s)
        want_d, want_s = np.zeros_like(gd), np.zeros_like(gs)
        want_d[row], want_s[row] = go_d[0], go_s[0]
        assert np.array_equal(gd, want_d) and np.array_equal(gs, want_s), pt

    one_row((2.0, 3.0, 4.0), links[2, 3, 4])      # exactly on a node: corner 000 with weight 1, the others add nothing
    one_row((5.0, 4.0, 6.0), links[5, 4, 6])      # the last node of every axis: l = size - 2, corner 111 with weight 1
    one_row((9.0, 40.0, 1e9), links[5, 4, 6])     # beyond the box on the upper sides: clamped onto it
    one_row((-3.0, -0.5, 2.0), links[0, 0, 2])    # beyond it on the lower sides
    for pt in ((-7.0, 2.5, 100.0), (3.25, -1.0, 2.5)):      # clamped on one side each: the clamped point's gradients, bit for bit
        clamped = np.clip(np.array(pt), 0.0, np.array(links.shape) - 1.0)
        got, want = sample_grads(m, [pt], go_d, go_s), sample_grads(m, [clamped], go_d, go_s)
        oracle = GA.sample_backward(g, [pt], go_d, go_s, grid_coords=True)
        assert all(np.array_equal(x, y) for x, y in zip(got, want)) and got[0].any()
        assert all(np.array_equal(x, y) for x, y in zip(got, oracle))      # one add per entry: the restatement's, bit for bit
    gd, gs = sample_grads(m, [(0.5, 0.5, 0.5)], go_d, go_s)      # all eight corners empty: nothing is added
    assert not gd.any() and not gs.any()
    # 4096 copies of one point. Its weights are products of quarters and its cotangents multiples of 1/16 below 8: a term has
    # at most 13 significant bits and every partial sum of 4096 of them at most 24, so fp32 adds them without rounding in any
    # order - the sum is 4096 x one contribution exactly, and an add lost to a race would show as 1 / 4096 of an entry.
    pt = (2.25, 3.5, 4.75)
    one = sample_grads(m, [pt], go_d, go_s)
    many = sample_grads(m, [pt] * 4096, np.repeat(go_d, 4096, 0), np.repeat(go_s, 4096, 0))
    assert (one[0] != 0).sum() == 8 and (one[1] != 0).sum() == 8 * 12
    assert np.array_equal(many[0], 4096.0 * one[0]) and np.array_equal(many[1], 4096.0 * one[1])
    # want_colors=False: the density column alone, and no gradient for sh_data
    gd0, gs0 = sample_grads(m, [pt], go_d, go_s, want_colors=False)
    assert np.array_equal(gd0, one[0]) and gs0 is None


# ---- 6. batch edges -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_case(basis_dim):
    """a small grid with kept faces, w + 1 rays through it (w = rays of a workgroup), a cotangent, skip distances"""
    rng = np.random.default_rng(800 + basis_dim)
    g = random_grid_with_faces(rng, (14, 12, 16), basis_dim, keep=0.4, sh_std=2.0)
    n = 256 // LANES[basis_dim] + 1
    o, d = through_rays(rng, g, n)
    return g, o, d, rng.normal(size=(n, 3)).astype(np.float32), GO.skip_distances(g["links"])


@pytest.mark.parametrize("basis_dim", [9, 4, 1])
def test_batch_sizes_around_a_wavefront_and_a_workgroup(N, basis_dim):
    g, o, d, cot, skip = edge_case(basis_dim)
    r, w = 64 // LANES[basis_dim], 256 // LANES[basis_dim]
    sizes = [r - 1, r, r + 1, w - 1, w, w + 1]
    assert sizes == {9: [1, 2, 3, 7, 8, 9], 4: [3, 4, 5, 15, 16, 17], 1: [15, 16, 17, 63, 64, 65]}[basis_dim]
    grid = make_grid(N, g)
    m = N.GridModule(grid)
    want = {n: GA.render_vjp(g, o[:n], d[:n], cot[:n], skip=skip) for n in sizes}
    for accelerated in (False, True):
        if accelerated:
            grid.accelerate()
        for n in sizes:
            label = f"B = {basis_dim} n = {n} {'accelerated' if accelerated else 'plain'}"
            rgb, gd, gs = vjp(m, o[:n], d[:n], cot[:n])
            assert np.abs(rgb - want[n][0]).max() <= 1e-5
            assert_close(label + " d/ddensity", gd, want[n][1])
            assert_close(label + " d/dsh", gs, want[n][2])


@pytest.mark.parametrize("basis_dim", [9, 4, 1])
def test_a_batch_is_the_sum_of_its_halves(N, basis_dim):
    g, o, d, cot, _ = edge_case(basis_dim)
    n = len(o)
    h = n // 2
    m = N.GridModule(make_grid(N, g))
    whole, first, second = vjp(m, o, d, cot), vjp(m, o[:h], d[:h], cot[:h]), vjp(m, o[h:], d[h:], cot[h:])
    assert np.array_equal(whole[0], np.concatenate([first[0], second[0]]))
    for i, key in ((1, "density"), (2, "sh")):
        assert_close(f"B = {basis_dim}: {n} rays vs {h} + {n - h}, d/d{key}", whole[i], first[i].astype(np.float64) + second[i])


def test_zero_rays_and_zero_points(N):
    g = hand_grid()
    m = N.GridModule(make_grid(N, g))
    empty = torch.zeros((0, 3), device="cuda")
    rgb = m.volume_render(N.Rays(empty, empty))
    assert rgb.shape == (0, 3) and rgb.requires_grad
    rgb.sum().backward()
    dens, sh = m.sample(empty)
    assert dens.shape == (0, 1) and sh.shape == (0, 12)
    (dens.sum() + sh.sum()).backward()
    assert not m.density_data.grad.any() and not m.sh_data.grad.any()
    assert m.density_data.grad.shape == m.density_data.shape and m.sh_data.grad.shape == m.sh_data.shape


@pytest.mark.parametrize("basis_dim", [9, 1])
def test_misses_and_hostile_rays_give_the_background_and_no_gradient(N, basis_dim):
    rng = np.random.default_rng(900 + basis_dim)
    g = random_grid(rng, (20, 18, 22), basis_dim, keep=0.4)
    grid = make_grid(N, g)
    set_opt(grid, 0.4, 0.5, 0.0)
    m = N.GridModule(grid)
    ho, hd = hostile_rays(g)
    # every ray of the batch misses or is not finite: the background, zero gradients, no NaN - whatever the cotangent holds
    for cot in (np.ones((8, 3), np.float32), np.full((8, 3), np.nan, np.float32)):
        rgb, gd, gs = vjp(m, ho, hd, cot)
        assert np.array_equal(rgb, np.full((8, 3), 0.4, np.float32)) and not gd.any() and not gs.any()
    # inside a batch they change nothing
    o64, d64 = through_rays(rng, g, 64)
    c64 = rng.normal(size=(64, 3)).astype(np.float32)
    where = np.array([0, 1, 2, 35, 36, 37, 70, 71])
    good = np.setdiff1d(np.arange(72), where)
    o, d, cot = np.zeros((72, 3), np.float32), np.zeros((72, 3), np.float32), np.full((72, 3), np.nan, np.float32)
    o[good], d[good], cot[good] = o64, d64, c64
    o[where], d[where] = ho, hd
    for accelerated in (False, True):
        if accelerated:
            grid.accelerate()
        base, got = vjp(m, o64, d64, c64), vjp(m, o, d, cot)
        assert np.array_equal(got[0][where], np.full((8, 3), 0.4, np.float32)) and np.array_equal(got[0][good], base[0])
        assert base[1].any() and base[2].any()
        assert_close(f"B = {basis_dim} hostile d/ddensity", got[1], base[1])
        assert_close(f"B = {basis_dim} hostile d/dsh", got[2], base[2])


# ---- 7. the module's contract -------------------------------------------------------------------------------------------
def test_module_behaviour(N):
    z = np.load(RENDER)
    g = fixture_grid(z, "b")
    grid = make_grid(N, g)
    grid.accelerate()
    m = N.GridModule(grid)
    o, d = z["b_origins"][:300], z["b_dirs"][:300]
    rays = N.Rays(gpu(o), gpu(d))
    assert [n for n, _ in m.named_parameters()] == ["density_data", "sh_data"]
    assert m.density_data.data_ptr() == grid.density_data.data_ptr() and m.sh_data.data_ptr() == grid.sh_data.data_ptr()
    assert not grid.density_data.requires_grad and not grid.sh_data.requires_grad and m.density_data.is_leaf
    # rgb.sum().backward() hands in a stride-0 expansion: the VJP with ones
    _, gd1, gs1 = vjp(m, o, d, np.ones((300, 3), np.float32))
    m.zero_grad(set_to_none=True)
    m.volume_render(rays).sum().backward()
    assert_close("sum().backward() d/ddensity", cpu(m.density_data.grad), gd1)
    assert_close("sum().backward() d/dsh", cpu(m.sh_data.grad), gs1)
    # ... and so does a transposed (non-contiguous) cotangent
    cot = torch.randn(3, 300, device="cuda").t()
    assert not cot.is_contiguous()
    _, gd2, gs2 = vjp(m, o, d, cpu(cot))
    m.zero_grad(set_to_none=True)
    m.volume_render(rays).backward(cot)
    assert_close("non-contiguous cotangent d/dsh", cpu(m.sh_data.grad), gs2)
    # gradients accumulate into .grad as torch's do
    m.volume_render(rays).backward(cot)
    assert_close("accumulated d/ddensity", cpu(m.density_data.grad), 2.0 * gd2.astype(np.float64))
    # a frozen parameter: no gradient there, the same one on the other; both frozen: the plain kernel, no graph
    for frozen, free, want in (("density_data", "sh_data", gs1), ("sh_data", "density_data", gd1)):
        m.zero_grad(set_to_none=True)
        getattr(m, frozen).requires_grad_(False)
        m.volume_render(rays).sum().backward()
        assert getattr(m, frozen).grad is None
        assert_close(f"{frozen} frozen, d/d{free}", cpu(getattr(m, free).grad), want)
        dens, sh = m.sample(gpu(z["b_pts_world"]))
        (dens.sum() + sh.sum()).backward()
        assert getattr(m, frozen).grad is None
        getattr(m, frozen).requires_grad_(True)
    m.requires_grad_(False)
    assert not m.volume_render(rays).requires_grad and not m.sample(gpu(z["b_pts_world"]))[0].requires_grad
    m.requires_grad_(True)
    # an in-place step between forward and backward: torch's version check refuses the backward
    m.zero_grad(set_to_none=True)
    rgb = m.volume_render(rays)
    with torch.no_grad():
        m.sh_data.add_(0.125)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        rgb.sum().backward()
    dens, _ = m.sample(gpu(z["b_pts_world"]))
    grid.density_data.mul_(1.0)      # through the grid's own tensor: the same version counter
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        dens.sum().backward()
    # refusals, in SparseGrid's vocabulary
    with pytest.raises(NotImplementedError, match="gradient"):
        m.volume_render(N.Rays(gpu(o).requires_grad_(True), gpu(d)))
    with pytest.raises(NotImplementedError, match="gradient"):
        m.sample(gpu(z["b_pts_world"]).requires_grad_(True))
    with pytest.raises(RuntimeError, match="CPU"):
        m.volume_render(N.Rays(torch.from_numpy(o), torch.from_numpy(d)))
    with pytest.raises(RuntimeError, match="CPU"):
        m.sample(torch.from_numpy(z["b_pts_world"]))
    with pytest.raises(ValueError):
        m.volume_render(N.Rays(gpu(o), gpu(d[:7])))
    with pytest.raises(ValueError):
        m.sample(gpu(o[:, :2]))
    for call in (lambda: m.volume_render(rays, use_kernel=False), lambda: m.sample(gpu(o), use_kernel=False),
                 lambda: m.volume_render_image(fixture_camera(N, z), use_kernel=False)):
        with pytest.raises(NotImplementedError, match="use_kernel"):
            call()
    assert grid.accelerated      # nothing above cost the grid its handle or its skip data
    # replaced tables: the next call names rebind(), and after it the module works on the new ones
    old_d = grid.density_data
    grid.density_data = old_d.clone()
    for call in (lambda: m.volume_render(rays), lambda: m.sample(gpu(o)), lambda: m.volume_render_image(fixture_camera(N, z))):
        with pytest.raises(RuntimeError, match=r"rebind\(\)"):
            call()
    m.sh_data.requires_grad_(False)
    assert m.rebind() is m and m.density_data.data_ptr() == grid.density_data.data_ptr() != old_d.data_ptr()
    assert m.density_data.requires_grad and not m.sh_data.requires_grad      # (what was frozen stays frozen)
    m.sh_data.requires_grad_(True)
    m.volume_render(rays).sum().backward()
    assert m.density_data.grad.abs().max() > 0 and m.sh_data.grad.abs().max() > 0
    trainer = N.GridTrainer(grid)
    trainer.resample([12, 12, 12], sigma_thresh=1.0, weight_thresh=0.0, dilate=1)
    with pytest.raises(RuntimeError, match=r"rebind\(\)"):
        m.volume_render(rays)
    m.rebind()
    assert m.sh_data.shape == grid.sh_data.shape and torch.equal(m.volume_render(rays), grid.volume_render(rays))


# ---- 8. a torch optimiser ---------------------------------------------------------------------------------------------
def test_adam_on_a_charbonnier_loss(N):
    z = np.load(RENDER)
    g = fixture_grid(z, "b")
    rays = N.Rays(gpu(z["b_origins"][:704]), gpu(z["b_dirs"][:704]))
    target = gpu(z["b_bg1_rgb64"][:704].astype(np.float32))
    start = dict(g, density_data=(np.float32(0.5) * g["density_data"]).astype(np.float32), sh_data=np.zeros_like(g["sh_data"]))
    grid = make_grid(N, start)
    set_opt(grid, 1.0, 0.5, 0.0, 0.0, 0.0)
    grid.accelerate()
    from nerf_projects_amd import synthetic
    cam = N.Camera.from_nerf_pose(synthetic.pose_spherical(40.0, -25.0, 3.5), 24, 32, 30.0)      # it looks at the grid
    before = grid.volume_render_image(cam).clone()
    assert (before != 1.0).any(dim=-1).float().mean() > 0.05
    handle = grid._handle().value
    m = N.GridModule(grid)
    adam = torch.optim.Adam([{"params": [m.density_data], "lr": 0.5}, {"params": [m.sh_data], "lr": 2e-2}])
    losses = []
    for _ in range(20):
        adam.zero_grad()
        loss = torch.sqrt((m.volume_render(rays) - target) ** 2 + 1e-3).mean()
        loss.backward()
        adam.step()
        losses.append(float(loss.detach()))
    print(f"Charbonnier, 20 Adam steps: {losses[0]:.5f} -> {losses[-1]:.5f}")
    assert losses[-1] < losses[0] and np.isfinite(losses).all()
    # the grid itself renders the trained values: the same handle, still accelerated, what a fresh grid of the same tables renders
    after = grid.volume_render_image(cam)
    assert grid._handle().value == handle and grid.accelerated
    assert not torch.equal(after, before)
    fresh = N.SparseGrid.from_tensors(grid.links.clone(), grid.density_data.clone(), grid.sh_data.clone(), g["radius"].tolist(),
                                      g["center"].tolist())
    fresh.opt = grid.opt
    assert torch.equal(after, fresh.volume_render_image(cam))
    assert torch.equal(m.density_data.detach(), grid.density_data) and not torch.equal(grid.density_data, gpu(start["density_data"]))


# ---- 9. the old pins, in the same process -------------------------------------------------------------------------------
def test_sparse_grid_itself_still_refuses_gradients(N):
    g = hand_grid()
    grid = make_grid(N, g)
    m = N.GridModule(grid)
    m.volume_render(N.Rays(*(gpu(x) for x in through_rays(np.random.default_rng(1), g, 8)))).sum().backward()
    with pytest.raises(NotImplementedError, match="gradients"):
        N.SparseGrid.from_tensors(gpu(g["links"]), gpu(g["density_data"]).requires_grad_(True), gpu(g["sh_data"]),
                                  g["radius"].tolist(), g["center"].tolist())
    with pytest.raises(NotImplementedError, match="gradients"):
        grid.volume_render(N.Rays(torch.zeros((4, 3), device="cuda", requires_grad=True), torch.ones((4, 3), device="cuda")))
    with pytest.raises(NotImplementedError, match="volume_render_fused"):
        grid.volume_render_fused()
    with pytest.raises(NotImplementedError):
        grid.volume_render(N.Rays(torch.zeros((4, 3), device="cuda"), torch.ones((4, 3), device="cuda")), use_kernel=False)
