"""Forward-facing scenes on the GPU: the NDC warp (``rays_to_ndc``), ``NdcCamera`` through every image call, the LLFF loader
and its NDC batches, against what the reference's svox2 recorded for tests/golden/tiny_scene/llff_svox2
(tests/golden/grid_ndc.npz, made by tests/golden/make_golden_grid_ndc.py). Rays are compared bit for bit; the render is held
to 3x the reference's own fp32 - fp64 distance."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest
import torch

import grid_oracle as GO
import grid_resample_oracle as RO
from test_grid import cpu, gpu, set_opt
from test_grid_cpu import bar
from test_grid_ndc_cpu import FIXTURE, ROOT

pytestmark = pytest.mark.gpu

SCENE = os.path.join(ROOT, "tests", "golden", "tiny_scene", "llff_svox2")
LLFF_JSON = os.path.join(ROOT, "tests", "golden", "svox2_configs", "llff.json")
N_CAMS = 5


@pytest.fixture(scope="module")
def N():
    import nerf_projects_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def Z():
    return dict(np.load(FIXTURE))


def ndc_camera(N, z, i, device="cuda"):
    fx, fy, cx, cy = z[f"cam{i}_intrinsics"].tolist()
    w, h = (int(v) for v in z[f"cam{i}_size"])
    c2w = torch.from_numpy(z[f"cam{i}_c2w"])
    return N.NdcCamera(c2w.to(device), fx, fy, cx, cy, width=w, height=h, ndc_coeffs=z[f"cam{i}_ndc_coeffs"].tolist())


def fixture_grid(z):
    return {"links": z["grid_links"], "density_data": z["grid_density"], "sh_data": z["grid_sh"],
            "radius": z["scene_radius"].astype(np.float32), "center": np.zeros(3, np.float32)}


def make_grid(N, z, density_scale=None):
    g = fixture_grid(z)
    dens = g["density_data"] if density_scale is None else (g["density_data"] * np.float32(density_scale)).astype(np.float32)
    grid = N.SparseGrid.from_tensors(gpu(g["links"]), gpu(dens), gpu(g["sh_data"]), g["radius"].tolist(), g["center"].tolist())
    set_opt(grid, 0.5, 0.5, 0.0)
    return grid


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 1. the warp ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [1, 2])
def test_rays_to_ndc_equals_the_reference_in_every_bit(N, Z, factor):
    coeffs = Z["ndc_coeffs"].tolist()
    wo, wd = Z[f"world_origins_{factor}"], Z[f"world_dirs_{factor}"]
    out = N.rays_to_ndc(N.Rays(gpu(wo), gpu(wd)), coeffs)
    assert isinstance(out, N.Rays) and out.origins.dtype == torch.float32 and out.origins.is_cuda
    o, d = cpu(out.origins), cpu(out.dirs)
    print(f"factor {factor}: {len(o)} rays, origins differ in {int((o != Z[f'ndc_origins_{factor}']).sum())} values, dirs in "
          f"{int((d != Z[f'ndc_dirs_{factor}']).sum())}")
    assert same_bits(o, Z[f"ndc_origins_{factor}"]) and same_bits(d, Z[f"ndc_dirs_{factor}"])


@pytest.mark.parametrize("n", [1, 65])
def test_rays_to_ndc_one_ray_and_one_past_a_wavefront_and_in_place(N, Z, n):
    coeffs = Z["ndc_coeffs"].tolist()
    wo, wd = Z["world_origins_1"][100:100 + n], Z["world_dirs_1"][100:100 + n]
    want_o, want_d = Z["ndc_origins_1"][100:100 + n], Z["ndc_dirs_1"][100:100 + n]
    # guard rows around the n rays: one lane per ray, nothing written past them
    o = torch.full((n + 2, 3), 7.0, device="cuda")
    d = torch.full((n + 2, 3), 9.0, device="cuda")
    o[1:-1], d[1:-1] = gpu(wo), gpu(wd)
    out = N.rays_to_ndc(N.Rays(o[1:-1], d[1:-1]), coeffs)
    assert same_bits(cpu(out.origins), want_o) and same_bits(cpu(out.dirs), want_d)
    # the C entry with each output aliasing its input
    from nerf_projects_amd import _lib
    from nerf_projects_amd.host import get_context
    ctx = get_context(o.device)
    a = _lib.GridRaysToNdcArgs()
    a.origins = a.origins_out = o[1:-1].data_ptr()
    a.dirs = a.dirs_out = d[1:-1].data_ptr()
    a.n = n
    a.ndc_coeffs[:] = coeffs
    a.stream = ctx.stream().value
    _lib.check(ctx.lib.nerf_grid_rays_to_ndc(ctx.handle, C.byref(a)))
    assert same_bits(cpu(o[1:-1]), want_o) and same_bits(cpu(d[1:-1]), want_d)
    assert (o[0] == 7.0).all() and (o[-1] == 7.0).all() and (d[0] == 9.0).all() and (d[-1] == 9.0).all()


def test_a_ray_parallel_to_the_image_plane_is_non_finite_and_a_miss(N, Z):
    coeffs = Z["ndc_coeffs"].tolist()
    o = gpu(np.array([[0.1, 0.2, 0.0], [0.0, 0.0, 0.0]], np.float32))
    d = gpu(np.array([[1.0, 0.5, 0.0], [0.0, 0.0, 1.0]], np.float32))      # dz == 0; and a good ray beside it
    out = N.rays_to_ndc(N.Rays(o, d), coeffs)
    assert not torch.isfinite(out.origins[0]).all() and not torch.isfinite(out.dirs[0]).all()
    assert torch.isfinite(out.origins[1]).all() and torch.isfinite(out.dirs[1]).all()
    grid = make_grid(N, Z)
    rgb, logt = grid.volume_render(out, return_log_transmit=True)
    assert (rgb[0] == 0.5).all() and float(logt[0]) == 0.0      # the background, nothing absorbed
    assert float(logt[1]) < -0.1      # the good ray goes down the middle of the box
    # argument errors
    with pytest.raises(ValueError, match="ndc_coeffs"):
        N.rays_to_ndc(N.Rays(o, d), (-1.0, -1.0))
    with pytest.raises(RuntimeError, match="CPU"):
        N.rays_to_ndc(N.Rays(o.cpu(), d.cpu()), coeffs)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        N.rays_to_ndc(N.Rays(o, d[:1]), coeffs)
    empty = N.rays_to_ndc(N.Rays(o[:0], d[:0]), coeffs)
    assert empty.origins.shape == (0, 3)


# ---- 2. NdcCamera.gen_rays ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(N_CAMS))
def test_ndc_camera_gen_rays_equals_the_reference_in_every_bit(N, Z, i):
    rays = ndc_camera(N, Z, i).gen_rays()
    o, d = cpu(rays.origins), cpu(rays.dirs)
    print(f"cam{i}: origins differ in {int((o != Z[f'cam{i}_origins']).sum())} values, dirs in {int((d != Z[f'cam{i}_dirs']).sum())}; "
          f"reference fp32 vs fp64 {float(Z[f'cam{i}_d_origins']):.2e} / {float(Z[f'cam{i}_d_dirs']):.2e}")
    assert same_bits(o, Z[f"cam{i}_origins"]) and same_bits(d, Z[f"cam{i}_dirs"])
    # a camera on the CPU makes the same rays on the default device
    rays = ndc_camera(N, Z, i, "cpu").gen_rays("cuda")
    assert same_bits(cpu(rays.dirs), Z[f"cam{i}_dirs"])


# ---- 3. image calls against ray calls -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sparse", "half", "half_pair", "palette"])
def test_image_calls_are_the_ray_calls_bit_for_bit(N, Z, kind):
    base = make_grid(N, Z)
    if kind == "sparse":
        grid = base
    elif kind == "palette":
        grid = N.PaletteGrid.from_grid(base, bits=6, retain=1)
    else:
        grid = N.HalfGrid.from_grid(base, lanes="pair" if kind == "half_pair" else "single")
    grid.opt = dataclasses.replace(base.opt)
    for accelerated in (False, True):
        if accelerated:
            grid.accelerate()
        assert grid.accelerated == accelerated
        for i in (0, 4):
            cam = ndc_camera(N, Z, i)
            rays = cam.gen_rays()
            img = grid.volume_render_image(cam)
            assert img.shape == (cam.height, cam.width, 3)
            assert torch.equal(img.view(-1, 3), grid.volume_render(rays)), (kind, accelerated, i)
            assert (img != 0.5).any()
            for thresh in (None, 2.0):
                depth = grid.volume_render_depth_image(cam, sigma_thresh=thresh)
                assert depth.shape == (cam.height, cam.width) and (depth > 0).any()
                assert torch.equal(depth.view(-1), grid.volume_render_depth(rays, sigma_thresh=thresh)), (kind, accelerated, i, thresh)


def test_grid_module_image_and_its_backward(N, Z):
    """The image form is the ray form of ``camera.gen_rays()``: the same forward bits, and the same backward. The backward adds
    its terms with fp32 atomics, so two runs over many rays may differ in the order of a sum. With a cotangent on ONE ray
    every address is written by one lane of one wavefront, sample after sample in program order: those are equal in every
    bit, and they are compared for rays from every part of the image."""
    cam = ndc_camera(N, Z, 4)
    n = cam.width * cam.height
    grid = make_grid(N, Z)
    module = N.GridModule(grid)
    rgb = module.volume_render_image(cam)
    assert rgb.requires_grad and torch.equal(rgb.detach(), grid.volume_render_image(cam))
    depth = module.volume_render_depth_image(cam)
    assert depth.requires_grad and torch.equal(depth.detach(), grid.volume_render_depth_image(cam))
    cot = torch.linspace(0.5, 1.5, 3 * n, device="cuda").view(n, 3)
    for ray in (0, cam.width - 1, n // 2, n // 2 + 5, n - cam.width, n - 1):
        one = torch.zeros_like(cot)
        one[ray] = cot[ray]
        grads = []
        for form in ("image", "rays"):
            module.zero_grad(set_to_none=True)
            out = module.volume_render_image(cam).view(n, 3) if form == "image" else module.volume_render(cam.gen_rays())
            (out * one).sum().backward()
            grads.append((module.density_data.grad.clone(), module.sh_data.grad.clone()))
        assert grads[0][0].abs().max() > 0 and grads[0][1].abs().max() > 0, ray
        assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1]), ray
    # every ray at once, and the depth with it: one backward through both image calls
    module.zero_grad(set_to_none=True)
    ((module.volume_render_image(cam).view(n, 3) * cot).sum() + module.volume_render_depth_image(cam).sum()).backward()
    assert torch.isfinite(module.density_data.grad).all() and torch.isfinite(module.sh_data.grad).all()
    assert (module.sh_data.grad != 0).any() and (module.density_data.grad != 0).any()


# ---- 4. parity against the reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["train", "cam4"])
def test_render_along_ndc_rays_against_the_reference(N, Z, tag):
    """3x the reference's own fp32 - fp64 distance, the bar of the existing render tests (tests/test_grid_cpu.py ``bar``)."""
    tol = bar(Z, "render")
    grid = make_grid(N, Z)
    set_opt(grid, 0.5, 0.5, 0.0, 0.0, 0.0)      # the PyTorch statement has no sigma_thresh and no early stop
    if tag == "train":
        rays = N.Rays(gpu(Z["ndc_origins_1"]), gpu(Z["ndc_dirs_1"]))
    else:
        rays = ndc_camera(N, Z, 4).gen_rays()
    got = cpu(grid.volume_render(rays))
    err = np.abs(got.astype(np.float64) - Z[f"render_{tag}_rgb"]).max(-1)
    print(f"render {tag}: GPU vs reference max {err.max():.3e} over {len(err)} rays (3 d_ref {3 * float(Z['render_d_ref']):.3e}, bar "
          f"{tol:.3e}); opacity > 0.1 on {(Z[f'render_{tag}_opacity64'] > 0.1).mean():.2f} of the rays")
    assert np.isfinite(got).all() and err.max() <= tol, (tag, int(err.argmax()), err.max())
    if tag == "cam4":
        img = cpu(grid.volume_render_image(ndc_camera(N, Z, 4))).reshape(-1, 3)
        assert np.abs(img.astype(np.float64) - Z["render_cam4_rgb"]).max() <= tol


# ---- 5. data set rays -----------------------------------------------------------------------------------------------------------
def fixture_dataset(N, z, **kw):
    fx, fy, cx, cy = z["intrins_full"].tolist()
    return N.GridDataset.from_arrays(z["images_u8"], z["c2w"], fx, fy, cx, cy, white_bkgd=False, ndc_coeffs=z["ndc_coeffs"].tolist(),
                                     **kw)


@pytest.mark.parametrize("factor", [1, 2])
def test_dataset_batches_equal_rays_init_in_every_bit(N, Z, factor):
    ds = fixture_dataset(N, Z, generator=torch.Generator(device="cpu").manual_seed(3))
    ds.gen_rays(factor)
    assert (ds.h, ds.w) == tuple(Z[f"hw_{factor}"]) and ds.n_rays == len(Z[f"ndc_origins_{factor}"])
    rays, rgb = ds.batch(0, ds.n_rays)
    o, d, c = cpu(rays.origins), cpu(rays.dirs), cpu(rgb)
    print(f"factor {factor}: {ds.n_rays} rays; values that differ: origins {int((o != Z[f'ndc_origins_{factor}']).sum())}, dirs "
          f"{int((d != Z[f'ndc_dirs_{factor}']).sum())}, colours {int((c != Z[f'gt_{factor}']).sum())}")
    assert same_bits(o, Z[f"ndc_origins_{factor}"]) and same_bits(d, Z[f"ndc_dirs_{factor}"]) and same_bits(c, Z[f"gt_{factor}"])
    # the camera of an image is an NdcCamera whose rays are the image's rows
    cam = ds.camera(2)
    assert isinstance(cam, N.NdcCamera) and (cam.height, cam.width) == (ds.h, ds.w)
    hw = ds.h * ds.w
    assert same_bits(cpu(ds.image(2)).reshape(-1, 3), Z[f"gt_{factor}"][2 * hw:3 * hw])
    # a new epoch: the rows at their indices
    ds.shuffle_rays()
    rays_s, rgb_s, idx = ds.batch(0, ds.n_rays, return_indices=True)
    idx = cpu(idx)
    assert sorted(idx.tolist()) == list(range(ds.n_rays)) and not np.array_equal(idx, np.arange(ds.n_rays))
    assert same_bits(cpu(rays_s.origins), o[idx]) and same_bits(cpu(rays_s.dirs), d[idx]) and same_bits(cpu(rgb_s), c[idx])
    part, _, idx_part = ds.batch(33, 91, return_indices=True)      # a batch that starts and ends inside wavefronts
    assert np.array_equal(cpu(idx_part), idx[33:91]) and same_bits(cpu(part.dirs), d[idx[33:91]])


def test_a_dataset_without_ndc_coeffs_is_unchanged(N, Z):
    fx, fy, cx, cy = Z["intrins_full"].tolist()
    ds = N.GridDataset.from_arrays(Z["images_u8"], Z["c2w"], fx, fy, cx, cy, white_bkgd=False)
    rays, _ = ds.batch(0, ds.n_rays)
    assert ds.ndc_coeffs == (-1, -1) and type(ds.camera(0)) is N.Camera
    assert same_bits(cpu(rays.origins), Z["world_origins_1"]) and same_bits(cpu(rays.dirs), Z["world_dirs_1"])
    with pytest.raises(ValueError, match="ndc_coeffs"):
        N.GridDataset.from_arrays(Z["images_u8"], Z["c2w"], fx, fy, cx, cy, ndc_coeffs=(1.0, -1.0))


# ---- 6. the loader ---------------------------------------------------------------------------------------------------------------
POSE_ATOL = 2e-6      # tests/test_datasets.py holds the same pose functions (recentring, spiral) to this


@pytest.mark.parametrize("hold_every", [8, 2])
@pytest.mark.parametrize("split", ["train", "test"])
def test_from_llff_against_the_reference_loader(N, Z, split, hold_every):
    offset = int(Z["offset"])
    ds = N.GridDataset.from_llff(SCENE, split, scale=0.5, hold_every=hold_every, offset=offset)
    want_c2w = Z[f"{split}_c2w_hold{hold_every}"]
    assert ds.n_images == len(want_c2w) == {("train", 8): 4, ("test", 8): 1, ("train", 2): 2, ("test", 2): 3}[(split, hold_every)]
    assert (ds.h_full, ds.w_full, ds.h, ds.w) == (8, 12, 8, 12) and ds.split == split
    it = ds.intrins_full
    assert np.array_equal(np.array([it.fx, it.fy, it.cx, it.cy]), Z["intrins_full"])
    assert np.array_equal(np.array(ds.ndc_coeffs), Z["ndc_coeffs"])
    assert np.array_equal(np.array(ds.scene_radius), Z["scene_radius"]) and ds.scene_center == [0.0, 0.0, 0.0]
    assert not ds.use_sphere_bound and not ds.white_bkgd and not ds.should_use_background
    np.testing.assert_allclose(np.array(ds.z_bounds), Z[f"{split}_z_bounds_hold{hold_every}"], rtol=0, atol=POSE_ATOL)
    err = np.abs(cpu(ds.c2w) - want_c2w).max()
    print(f"{split}, hold_every {hold_every}: {ds.n_images} views, c2w max error {err:.2e}")
    assert ds.c2w.shape == want_c2w.shape and err <= POSE_ATOL
    if split == "test":
        want = Z[f"render_c2w_hold{hold_every}"]
        assert ds.render_c2w.shape == want.shape == (120, 4, 4) and ds.render_c2w.is_cuda
        assert np.abs(cpu(ds.render_c2w) - want).max() <= POSE_ATOL
    else:
        assert not hasattr(ds, "render_c2w")
    if (split, hold_every) == ("train", 8):
        assert np.array_equal(cpu(ds.images_u8), Z["images_u8"])
        _, rgb = ds.batch(0, ds.n_rays)
        assert same_bits(cpu(rgb), Z["gt_1"])
        assert isinstance(ds.camera(0), N.NdcCamera)


def test_from_llff_refuses_what_it_cannot_read(N, tmp_path):
    with pytest.raises(NotImplementedError, match="INTER_AREA"):
        N.GridDataset.from_llff(SCENE, "train", scale=0.3)      # not integral
    with pytest.raises(NotImplementedError, match="INTER_AREA"):
        N.GridDataset.from_llff(SCENE, "train", scale=0.25)      # integral, but there is no images_4
    with pytest.raises(NotImplementedError, match="INTER_AREA"):
        N.GridDataset.from_llff(SCENE, "train")      # svox2's default, 1/4
    with pytest.raises(FileNotFoundError):
        N.GridDataset.from_llff(str(tmp_path / "nothing"), "train")
    with pytest.raises(ValueError, match="hold_every"):
        N.GridDataset.from_llff(SCENE, "train", scale=0.5, hold_every=0)
    with pytest.raises(ValueError, match="no view|no training view"):
        N.GridDataset.from_llff(SCENE, "train", scale=0.5, hold_every=1)
    full = N.GridDataset.from_llff(SCENE, "train", scale=1)      # images/ itself, 16 x 24
    assert (full.h_full, full.w_full, full.n_images) == (16, 24, 4)


# ---- 7. resampling with NDC cameras -------------------------------------------------------------------------------------------
def test_resample_keeps_the_nodes_the_restatement_keeps_for_the_recorded_rays(N, Z, monkeypatch):
    g = fixture_grid(Z)
    g["density_data"] = (g["density_data"] * np.float32(0.1)).astype(np.float32)      # rays reach the inside before they stop
    grid = make_grid(N, Z, density_scale=0.1)
    reso, thr = [20, 18, 8], 0.01
    ids = (0, 4)
    recorded = {(int(Z[f"cam{i}_size"][0]), int(Z[f"cam{i}_size"][1])): (Z[f"cam{i}_origins"], Z[f"cam{i}_dirs"]) for i in ids}
    # the restatement makes a camera's rays with grid_oracle.gen_rays: hand it the reference's recorded NDC rays instead
    monkeypatch.setattr(GO, "gen_rays", lambda c2w, fx, fy, cx, cy, w, h: recorded[(int(w), int(h))])
    dicts = [dict(c2w=None, fx=0, fy=0, cx=0, cy=0, width=int(Z[f"cam{i}_size"][0]), height=int(Z[f"cam{i}_size"][1])) for i in ids]
    want32 = RO.resample(g, reso, weight_thresh=thr, dilate_steps=0, cameras=dicts)
    want64 = RO.resample(g, reso, weight_thresh=thr, dilate_steps=0, cameras=dicts, dtype=np.float64)
    w32, w64 = want32["max_weight"], want64["max_weight"]
    bar = 3.0 * float(np.abs(w32.astype(np.float64) - w64).max())
    cams = [ndc_camera(N, Z, i) for i in ids]
    new = N.resample_grid(grid, reso, weight_thresh=thr, dilate=0, cameras=cams, accelerate=False)
    kept = cpu(new.links) >= 0
    m64 = w64 >= thr
    flips = kept != m64
    print(f"NDC resample {reso}: the restatement keeps {int(m64.sum())} of {m64.size} nodes, the GPU {int(kept.sum())}, flips "
          f"{int(flips.sum())} (bar on the weight {bar:.3e})")
    assert 0.05 * m64.size < m64.sum() < 0.95 * m64.size
    assert (np.abs(w64[flips] - thr) <= bar).all() and flips.sum() <= 1e-3 * m64.size + 1
    # the trainer's resample takes the same cameras
    trainer = N.GridTrainer(make_grid(N, Z, density_scale=0.1))
    trainer.resample(reso, weight_thresh=thr, dilate=0, cameras=cams)
    assert np.array_equal(cpu(trainer.grid.links) >= 0, kept)


# ---- 8. the driver --------------------------------------------------------------------------------------------------------------
def test_train_grid_on_the_llff_scene_with_llff_json(N, Z):
    offset = int(Z["offset"])
    gen = torch.Generator(device="cpu").manual_seed(11)
    train = N.GridDataset.from_llff(SCENE, "train", scale=0.5, offset=offset, generator=gen)
    test = N.GridDataset.from_llff(SCENE, "test", scale=0.5, offset=offset)
    cfg = dataclasses.replace(N.GridTrainConfig.from_json(LLFF_JSON), reso=[[12, 10, 6], [24, 20, 6]], upsamp_every=100, n_iters=200,
                              batch_size=96)
    seen = []
    real_camera = test.camera
    test.camera = lambda i: seen.append(real_camera(i)) or seen[-1]
    grid, history = N.train_grid(train, cfg, test=test, generator=torch.Generator(device="cpu").manual_seed(12))
    steps = [h for h in history if h["kind"] == "train"]
    evals = [h for h in history if h["kind"] == "eval"]
    # 384 rays in batches of 96: an entry per epoch of 4 steps; the first and the last 20 steps are 5 entries each
    assert len(steps) == 50 and steps[-1]["step"] == 199
    first, last = np.mean([h["mse"] for h in steps[:5]]), np.mean([h["mse"] for h in steps[-5:]])
    print(f"llff.json on 12 x 10 x 6 -> 24 x 20 x 6: batch mse {first:.5f} -> {last:.5f}; eval psnr {evals[0]['psnr']:.2f} -> "
          f"{evals[-1]['psnr']:.2f}; {grid.capacity} rows")
    assert list(grid.links.shape) == [24, 20, 6] and grid.capacity > 0      # it resampled once
    assert grid.radius.tolist() == np.array(train.scene_radius, np.float32).tolist()
    assert evals and all(isinstance(c, N.NdcCamera) for c in seen) and len(seen) >= len(evals)
    assert np.isfinite(last) and last < first


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------
def test_what_refuses_an_ndc_camera(N, Z):
    grid = make_grid(N, Z)
    cam = ndc_camera(N, Z, 0)
    labels = torch.ones(tuple(grid.links.shape), dtype=torch.int32, device="cuda")
    labels[:, :, :3] = 2
    fdr = {"floater_mask_3d": labels, "floater_component_ids": [2], "main_component_ids": [1], "num_components": 2}
    rgb = torch.zeros((cam.height, cam.width, 3), device="cuda")
    for fn in (lambda: N.project_floaters_to_view(grid, fdr, cam), lambda: N.component_view(grid, fdr, cam),
               lambda: N.multi_object_overlay(rgb, grid, fdr, cam)):
        with pytest.raises(NotImplementedError, match="NDC"):
            fn()
    bg = N.BackgroundGrid(reso=[6, 8, 4], basis_dim=4, background_nlayers=3, background_reso=4)
    with pytest.raises(NotImplementedError, match="NDC"):
        bg.volume_render_image(cam)
    assert torch.isfinite(bg.volume_render(cam.gen_rays())).all()      # rays of any kind stay welcome
    # Camera itself keeps refusing: the capability has its own name
    old = N.Camera(cam.c2w, cam.fx, cam.fy, cam.cx, cam.cy, width=cam.width, height=cam.height, ndc_coeffs=(1, 1))
    for fn in (old.gen_rays, lambda: grid.volume_render_image(old), lambda: grid.volume_render_depth_image(old),
               lambda: N.resample_grid(grid, [12, 10, 6], cameras=[old])):
        with pytest.raises(NotImplementedError, match="NDC"):
            fn()
    with pytest.raises(ValueError, match="ndc_coeffs"):
        N.NdcCamera(cam.c2w, cam.fx, width=4, height=4)      # the default (-1, -1)
    assert torch.isfinite(grid.volume_render_image(cam)).all()
