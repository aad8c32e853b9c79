"""Background layers of the sparse voxel grid on the GPU (include/nerf_mi355x.h, "Sparse voxel grid: background layers";
nerf-projects_amd/grid_background.py): the rendered colour and log_transmit of every fixture ray against the fp64 oracle,
bit-identity of the image form, of accelerated grids and of repeated runs, the rays the pass leaves alone, thinning against
its numpy statement, files, refusals and the inherited foreground-only calls. Needs a real MI355X: run with ``pytest -m gpu``.

Bounds: the colour within ``max(3 d_ref_rgb, 1e-5)`` and log_transmit within ``max(3 d_ref, 1e-5)``, with ``d_ref_rgb`` /
``d_ref`` the largest |oracle fp32 - oracle fp64| of the colour / of colour and log_transmit over the fixture
(tests/golden/make_golden_grid_background.py): the distance of an independent restatement from exact arithmetic, never of
the kernel."""
import os

import numpy as np
import pytest
import torch

import grid_background_oracle as BO
from test_grid import cpu, gpu, set_opt
from test_grid_background_cpu import BG_RESO, RESO, fixture_background, fixture_settings, load_fixture

pytestmark = pytest.mark.gpu

F, D = np.float32, np.float64


@pytest.fixture(scope="module")
def N():
    import nerf_projects_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def Z():
    return load_fixture()


def make_grid(N, Z, nlayers, bg=None):
    """a fresh BackgroundGrid on the fixture's foreground and the background of ``nlayers`` layers (or ``bg``)"""
    bg = fixture_background(Z, nlayers) if bg is None else bg
    return N.BackgroundGrid.from_tensors(gpu(Z["links"]), gpu(Z["density"]), gpu(Z["sh"]), Z["radius"].tolist(), Z["center"].tolist(),
                                         background_links=gpu(bg["links"]), background_data=gpu(bg["data"]))


def rays_of(N, Z):
    return N.Rays(gpu(Z["origins"]), gpu(Z["dirs"]))


def set_options(grid, Z, step, stop, brightness=None):
    set_opt(grid, float(Z["brightness"]) if brightness is None else brightness, step, 0.0, 1e-10, stop)


@pytest.fixture(scope="module")
def renders(N, Z):
    """``renders(j)`` -> (grid, rgb, log_transmit) of setting ``j`` as numpy, rendered once and never modified by a test"""
    made = {}

    def get(j):
        if j not in made:
            _, nl, step, stop = fixture_settings(Z)[j]
            g = make_grid(N, Z, nl)
            set_options(g, Z, step, stop)
            rgb, logt = g.volume_render(rays_of(N, Z), return_log_transmit=True)
            made[j] = (g, cpu(rgb), cpu(logt))
        return made[j]
    return get


@pytest.mark.parametrize("j", range(8))
def test_volume_render_meets_the_fp64_oracle_on_every_ray(N, Z, renders, j):
    _, nl, step, stop = fixture_settings(Z)[j]
    g, rgb, logt = renders(j)
    fg = g.foreground()
    set_options(fg, Z, step, stop, brightness=0.0)
    fg_rgb, fg_logt = (cpu(t) for t in fg.volume_render(rays_of(N, Z), return_log_transmit=True))
    # the foreground is tested elsewhere; here it must be what the fixture's generator saw, up to its own rounding
    assert np.abs(fg_rgb - Z[f"set{j}_fg_rgb"]).max() <= 1e-5
    assert ((fg_logt < -25) == (Z[f"set{j}_fg_logt"] < -25)).all()
    want_rgb, want_logt, st = BO.background_pass(Z["setup_o"], Z["setup_d"], Z["setup_delta_scale"], Z["setup_ok"], RESO,
                                                 fixture_background(Z, nl), fg_rgb, fg_logt, step, stop, float(Z["brightness"]), D,
                                                 return_stats=True)
    assert st["left_alone"].sum() >= 16 and st["brightness_only"].sum() >= 8 and (st["shaded"] > 0).sum() >= 200
    err_rgb = np.abs(rgb.astype(D) - want_rgb).max(-1)
    err_log = np.abs(logt.astype(D) - want_logt)
    bound_rgb, bound_log = max(3 * float(Z["d_ref_rgb"]), 1e-5), max(3 * float(Z["d_ref"]), 1e-5)
    print(f"setting {j}: L={nl} step={step} stop={stop}: rgb err max {err_rgb.max():.3e} (bound {bound_rgb:.3e}), log_T err max "
          f"{err_log.max():.3e} (bound {bound_log:.3e}), stopped {int(st['stopped'].sum())}, left alone {int(st['left_alone'].sum())}")
    assert np.isfinite(rgb).all() and np.isfinite(logt).all()
    assert (err_rgb <= bound_rgb).all(), (np.argwhere(err_rgb > bound_rgb)[:8].ravel(), err_rgb.max())
    assert (err_log <= bound_log).all(), (np.argwhere(err_log > bound_log)[:8].ravel(), err_log.max())
    # a ray the pass leaves alone keeps the foreground's bits; a ray that is not finite gets the brightness and nothing else
    assert np.array_equal(rgb[st["left_alone"]], fg_rgb[st["left_alone"]]) and np.array_equal(logt[st["left_alone"]], fg_logt[st["left_alone"]])
    only = st["brightness_only"]
    assert (logt[only] == 0).all() and np.array_equal(rgb[only], np.full((int(only.sum()), 3), F(Z["brightness"]), F))


def fixture_camera(N):
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grid_render.npz"))
    fx, fy, cx, cy = z["cam_intrinsics"]
    return N.Camera(torch.from_numpy(z["cam_c2w"]), fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy), width=24, height=16)


@pytest.mark.parametrize("j", [3, 6])
def test_image_is_bit_identical_to_the_cameras_rays(N, Z, renders, j):
    g = renders(j)[0]
    cam = fixture_camera(N)
    img = g.volume_render_image(cam)
    assert tuple(img.shape) == (16, 24, 3)
    rgb = g.volume_render(cam.gen_rays())
    assert torch.equal(img.view(-1, 3), rgb)
    fg = g.foreground()
    assert not torch.equal(fg.volume_render(cam.gen_rays()), rgb)      # the layers are in the frame
    # a camera whose sides are no multiple of the 8 x 8 tile, and one smaller than a tile
    for w, h in ((13, 9), (5, 3)):
        small = N.Camera(cam.c2w, fx=cam.fx * w / 24, fy=cam.fy * h / 16, cx=w * 0.47, cy=h * 0.54, width=w, height=h)
        assert torch.equal(g.volume_render_image(small).view(-1, 3), g.volume_render(small.gen_rays()))


@pytest.mark.parametrize("j", [1, 4])
def test_accelerated_equals_plain_and_two_runs_are_identical(N, Z, renders, j):
    _, nl, step, stop = fixture_settings(Z)[j]
    _, rgb, logt = renders(j)
    g = make_grid(N, Z, nl)
    set_options(g, Z, step, stop)
    g.accelerate()
    assert g.accelerated
    for _ in range(2):
        a, b = g.volume_render(rays_of(N, Z), return_log_transmit=True)
        assert np.array_equal(cpu(a), rgb) and np.array_equal(cpu(b), logt)
    assert g.accelerated


@pytest.mark.parametrize("j", [2, 7])
def test_a_background_without_positive_sigma_is_the_foregrounds_brightness_term(N, Z, j):
    _, nl, step, stop = fixture_settings(Z)[j]
    bg = fixture_background(Z, nl)
    bg = {"links": bg["links"], "data": bg["data"].copy()}
    bg["data"][..., 3] = -np.abs(bg["data"][..., 3])
    bg["data"][::3, :, 3] = 0.0
    g = make_grid(N, Z, nl, bg)
    fg = g.foreground()
    for grid in (g, fg):
        set_options(grid, Z, step, stop)
    rgb, logt = (cpu(t) for t in g.volume_render(rays_of(N, Z), return_log_transmit=True))
    want, want_logt = (cpu(t) for t in fg.volume_render(rays_of(N, Z), return_log_transmit=True))
    assert np.array_equal(logt, want_logt)
    lit = want_logt >= -25
    assert lit.sum() >= 200 and (~lit).sum() >= 16
    assert np.array_equal(rgb[lit], want[lit])
    assert np.abs(rgb[~lit].astype(D) - want[~lit]).max() <= 2e-11 * float(Z["brightness"])


# ---- thinning -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nl,thresh,dilate", [(5, 5.9, 1), (8, 5.5, 0), (2, 5.9, 2)])      # 48 of 103, 49 of 101, 44 of 87 rows stay
def test_sparsify_background_against_its_numpy_statement(N, Z, nl, thresh, dilate):
    bg = fixture_background(Z, nl)
    g = make_grid(N, Z, nl)
    set_options(g, Z, 0.5, 1e-7)
    g.accelerate()
    alias = g.background_links
    kept = g.sparsify_background(thresh, dilate)
    want_links, want_data = BO.sparsify(bg, thresh, dilate)
    assert 0 < kept == want_data.shape[0] < bg["data"].shape[0]
    assert g.background_links is alias and g.background_links.dtype == torch.int32      # in place
    assert np.array_equal(cpu(g.background_links), want_links)
    assert np.array_equal(cpu(g.background_data), want_data) and g.background_data.shape[0] == kept
    assert g.accelerated      # the foreground's skip data survives
    # the render after it = the render with the dropped texels' links set to -1 by hand
    by_hand = {"links": np.where(want_links >= 0, bg["links"], -1).astype(np.int32), "data": bg["data"]}
    h = make_grid(N, Z, nl, by_hand)
    set_options(h, Z, 0.5, 1e-7)
    a = g.volume_render(rays_of(N, Z), return_log_transmit=True)
    b = h.volume_render(rays_of(N, Z), return_log_transmit=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_sparsify_background_that_drops_nothing_leaves_the_render_unchanged(N, Z, renders):
    j = 2
    _, nl, step, stop = fixture_settings(Z)[j]
    _, rgb, logt = renders(j)
    g = make_grid(N, Z, nl)
    set_options(g, Z, step, stop)
    n_rows = g.background_data.shape[0]
    assert g.sparsify_background(sigma_thresh=-2.0, dilate=0) == n_rows
    links = cpu(g.background_links)
    assert np.array_equal(links[links >= 0], np.arange(n_rows))      # C order now
    a, b = g.volume_render(rays_of(N, Z), return_log_transmit=True)
    assert np.array_equal(cpu(a), rgb) and np.array_equal(cpu(b), logt)
    assert g.sparsify_background(sigma_thresh=1e9, dilate=3) == 0      # and a threshold above everything drops every row
    assert (cpu(g.background_links) == -1).all() and tuple(g.background_data.shape) == (0, nl, 4)
    fg = g.foreground()
    set_options(fg, Z, step, stop)
    c = g.volume_render(rays_of(N, Z))
    want = cpu(fg.volume_render(rays_of(N, Z), return_log_transmit=True)[1]) >= -25
    assert np.array_equal(cpu(c)[want], cpu(fg.volume_render(rays_of(N, Z)))[want])


def test_sparsify_background_over_several_compaction_blocks(N, Z):
    """2 * 40^2 = 3200 texels: four workgroups of the compaction, the last one partial; a tenth of the texels has no row."""
    rng = np.random.default_rng(5)
    R, nl = 40, 3
    texels = 2 * R * R
    has = rng.random(texels) >= 0.1
    links = np.full(texels, -1, np.int32)
    links[has] = rng.permutation(int(has.sum())).astype(np.int32)
    data = rng.uniform(-1, 2, (int(has.sum()), nl, 4)).astype(F)
    bg = {"links": links.reshape(2 * R, R), "data": data}
    g = make_grid(N, Z, nl, bg)
    kept = g.sparsify_background(1.6, 1)
    want_links, want_data = BO.sparsify(bg, 1.6, 1)
    assert 100 < kept == want_data.shape[0] < data.shape[0]
    assert np.array_equal(cpu(g.background_links), want_links) and np.array_equal(cpu(g.background_data), want_data)


# ---- the borrowed tensors ---------------------------------------------------------------------------------------------------
def test_writes_to_the_background_tensors_are_seen_by_the_next_call(N, Z):
    nl = 5
    bg = fixture_background(Z, nl)
    g = make_grid(N, Z, nl)
    set_options(g, Z, 0.5, 1e-7)
    rays = rays_of(N, Z)
    before = g.volume_render(rays)
    g.accelerate()
    g.background_links[4:12] = -1      # in place, through the property
    cut = {"links": bg["links"].copy(), "data": bg["data"]}
    cut["links"][4:12] = -1
    h = make_grid(N, Z, nl, cut)
    set_options(h, Z, 0.5, 1e-7)
    after = g.volume_render(rays)
    assert torch.equal(after, h.volume_render(rays)) and not torch.equal(after, before)
    assert g.accelerated      # re-attaching the background does not make a new handle
    g.background_data = gpu(bg["data"] * F(0.5))
    assert not torch.equal(g.volume_render(rays), after)
    g.background_links[0, 0] = bg["data"].shape[0]      # a row that does not exist
    with pytest.raises(RuntimeError, match="capacity"):
        g.volume_render(rays)
    g.background_links[0, 0] = -1
    g.volume_render(rays)
    assert g.use_background and g.background_nlayers == nl and g.background_reso == BG_RESO


def test_constructor_from_grid_and_argument_errors(N, Z):
    g = N.BackgroundGrid(reso=[6, 8, 4], basis_dim=4, background_nlayers=3, background_reso=4)
    assert tuple(g.background_links.shape) == (8, 4) and tuple(g.background_data.shape) == (32, 3, 4)
    assert np.array_equal(cpu(g.background_links).ravel(), np.arange(32)) and not cpu(g.background_data).any()
    assert g.use_background and g.background_nlayers == 3 and g.background_reso == 4 and g.links.shape == (6, 8, 4)
    g.opt.background_brightness = 0.25
    rays = N.Rays(gpu(Z["origins"][:64]), gpu(Z["dirs"][:64]))
    rgb = cpu(g.volume_render(rays))      # an empty scene: the brightness
    assert np.array_equal(rgb, np.full((64, 3), F(0.25)))
    fg = g.foreground()
    assert type(fg) is N.SparseGrid and fg.links is g.links and fg.sh_data is g.sh_data and not fg.use_background
    b = N.BackgroundGrid.from_grid(fg, 4, 6)
    assert b.links is fg.links and b.density_data is fg.density_data and tuple(b.background_data.shape) == (72, 4, 4)
    assert b.opt == fg.opt and b.opt is not fg.opt
    with pytest.raises(TypeError):
        N.BackgroundGrid.from_grid(fg.to_half(), 4, 6)
    good = fixture_background(Z, 5)

    def build(links=None, data=None):
        return N.BackgroundGrid.from_tensors(gpu(Z["links"]), gpu(Z["density"]), gpu(Z["sh"]), [1.0] * 3, [0.0] * 3,
                                             background_links=gpu(good["links"]) if links is None else links,
                                             background_data=gpu(good["data"]) if data is None else data)
    with pytest.raises(RuntimeError, match="CPU"):
        build(links=torch.from_numpy(good["links"]))
    with pytest.raises(RuntimeError, match="CPU"):
        build(data=torch.from_numpy(good["data"]))
    with pytest.raises(TypeError, match="int32"):
        build(links=gpu(good["links"].astype(np.int64)))
    with pytest.raises(TypeError, match="float32"):
        build(data=gpu(good["data"].astype(np.float16)))
    with pytest.raises(ValueError, match="2 R, R"):
        build(links=gpu(good["links"][:15]))
    with pytest.raises(ValueError, match="capacity, L, 4"):
        build(data=gpu(good["data"][..., :3]))
    with pytest.raises(ValueError, match="at least 2"):
        build(data=gpu(good["data"][:, :1]))
    with pytest.raises(ValueError, match="contiguous"):
        build(links=gpu(np.ascontiguousarray(good["links"].T)).T)
    with pytest.raises(NotImplementedError, match="training"):
        build(data=gpu(good["data"]).requires_grad_())
    with pytest.raises(RuntimeError, match="capacity"):
        build(data=gpu(good["data"][:-1]))


def test_c_calls_on_real_handles_attach_detach_and_refuse(N, Z):
    import ctypes as C
    from nerf_projects_amd import _lib
    g = make_grid(N, Z, 5)
    lib, h = g.ctx.lib, g._handle()
    err = lambda: lib.nerf_last_error().decode()      # noqa: E731
    assert lib.nerf_grid_has_background(h) == 1
    rays = rays_of(N, Z)
    rgb, logt = gpu(np.zeros((512, 3), F)), gpu(np.zeros(512, F))
    opt = g.opt._to_c()
    a = _lib.GridBackgroundArgs()
    a.origins, a.dirs, a.n_rays = rays.origins.data_ptr(), rays.dirs.data_ptr(), 512
    a.rgb, a.log_transmit, a.stream = rgb.data_ptr(), logt.data_ptr(), g.ctx.stream().value
    assert lib.nerf_grid_background_rays(h, C.byref(opt), C.byref(a)) == 0
    assert float(rgb.abs().sum()) > 0
    assert lib.nerf_grid_set_background(h, None) == 0 and lib.nerf_grid_has_background(h) == 0      # NULL detaches
    assert lib.nerf_grid_background_rays(h, C.byref(opt), C.byref(a)) == -1 and "no background" in err()
    g.background_links = g.background_links.clone()      # (so that the object attaches it again)
    half = g.foreground().to_half()
    d = _lib.GridBackgroundDesc()
    d.nlayers, d.reso, d.capacity = 5, BG_RESO, int(g.background_data.shape[0])
    d.links, d.data, d.stream = g.background_links.data_ptr(), g.background_data.data_ptr(), g.ctx.stream().value
    assert lib.nerf_grid_set_background(half._handle(), C.byref(d)) == -1 and "half-precision" in err()
    assert lib.nerf_grid_has_background(half._handle()) == 0
    assert lib.nerf_grid_set_background(g._handle(), C.byref(d)) == 0 and lib.nerf_grid_has_background(h) == 1


def test_an_empty_batch_renders_nothing(N, Z, renders):
    g = renders(5)[0]
    empty = N.Rays(gpu(np.zeros((0, 3), F)), gpu(np.zeros((0, 3), F)))
    rgb, logt = g.volume_render(empty, return_log_transmit=True)
    assert tuple(rgb.shape) == (0, 3) and tuple(logt.shape) == (0,)


# ---- files, refusals, what is inherited ----------------------------------------------------------------------------------
def test_save_and_load_grid_round_trip_renders_identical_bits(N, Z, renders, tmp_path):
    j = 6
    _, nl, step, stop = fixture_settings(Z)[j]
    g, rgb, logt = renders(j)
    p = str(tmp_path / "scene.npz")
    g.save(p)
    z = np.load(p)
    assert z["background_links"].dtype == np.int32 and z["background_links"].shape == (2 * BG_RESO, BG_RESO)
    assert z["background_data"].dtype == F and z["background_data"].shape[1:] == (nl, 4)
    back = N.load_grid(p)
    assert type(back) is N.BackgroundGrid and back.background_nlayers == nl and back.background_reso == BG_RESO
    set_options(back, Z, step, stop)
    a, b = back.volume_render(rays_of(N, Z), return_log_transmit=True)
    assert np.array_equal(cpu(a), rgb) and np.array_equal(cpu(b), logt)
    q = str(tmp_path / "plain.npz")
    g.foreground().save(q)
    assert type(N.load_grid(q)) is N.SparseGrid
    with pytest.raises(ValueError, match="SparseGrid.load"):
        N.BackgroundGrid.load(q)
    with pytest.raises(NotImplementedError, match="background"):
        N.SparseGrid.load(p)


def test_foreground_only_tools_refuse_and_name_foreground(N, Z, renders):
    g = renders(0)[0]
    for call in (lambda: N.GridTrainer(g), lambda: N.GridModule(g), lambda: N.resample_grid(g, 8), lambda: N.remove_floaters(g),
                 lambda: g.to_half(), lambda: N.HalfGrid.from_grid(g)):
        with pytest.raises(NotImplementedError, match=r"foreground\(\)"):
            call()
    N.GridTrainer(g.foreground())      # and the foreground is taken


def test_depth_and_ray_length_are_the_foregrounds(N, Z, renders):
    g = renders(4)[0]
    fg = g.foreground()
    fg.opt = g.opt
    rays = rays_of(N, Z)
    for got, want in ((g.volume_render_depth(rays), fg.volume_render_depth(rays)),
                      (g.volume_render_depth(rays, sigma_thresh=2.0), fg.volume_render_depth(rays, sigma_thresh=2.0)),
                      (g.volume_render(rays, return_raylen=True), fg.volume_render(rays, return_raylen=True))):
        assert torch.equal(got, want) or np.array_equal(cpu(got), cpu(want), equal_nan=True)
    cam = fixture_camera(N)
    assert torch.equal(g.volume_render_depth_image(cam), fg.volume_render_depth_image(cam))
    d, s = g.sample(gpu(Z["origins"][:64]))
    d2, s2 = fg.sample(gpu(Z["origins"][:64]))
    assert np.array_equal(cpu(d), cpu(d2), equal_nan=True) and np.array_equal(cpu(s), cpu(s2), equal_nan=True)
    assert g.count_samples(rays=rays) == fg.count_samples(rays=rays)


def test_a_table_of_the_tanks_and_temples_size_is_indexed_past_2_31_bytes(N, Z):
    """2048 x 1024 texels of 64 layers: 2 GiB of rows, so a row's byte offset passes 2^31. The same scene with its rows in
    reverse order must render the same bits; under 32-bit offsets the two would read different memory."""
    R, nl = 1024, 64
    cap = 2 * R * R
    gen = torch.Generator(device="cuda").manual_seed(11)
    data = torch.rand((cap, nl, 4), device="cuda", generator=gen) * 3.0 - 1.0
    links = torch.arange(cap, dtype=torch.int32, device="cuda").view(2 * R, R)
    fwd = N.BackgroundGrid.from_tensors(gpu(Z["links"]), gpu(Z["density"]), gpu(Z["sh"]), Z["radius"].tolist(), Z["center"].tolist(),
                                        background_links=links, background_data=data)
    rays = rays_of(N, Z)
    a = fwd.volume_render(rays, return_log_transmit=True)
    rev = N.BackgroundGrid.from_tensors(fwd.links, fwd.density_data, fwd.sh_data, Z["radius"].tolist(), Z["center"].tolist(),
                                        background_links=(cap - 1 - links).contiguous(), background_data=data.flip(0).contiguous())
    b = rev.volume_render(rays, return_log_transmit=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.isfinite(a[0]).all() and float((a[1] < -0.5).float().mean()) > 0.3      # the layers were composited
