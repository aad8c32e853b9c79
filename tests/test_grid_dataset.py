"""Sparse voxel grid training data on the GPU: the batch kernel against its numpy oracle (and through it against the
reference's recorded rays, tests/test_grid_dataset_cpu.py), ``GridDataset``'s surface and refusals, and ``train_grid`` on
the committed tiny scene. Needs a real MI355X: run with ``pytest -m gpu``."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_dataset_oracle as DO  # noqa: E402
import grid_fit_testlib as FT  # noqa: E402
from test_grid_dataset_cpu import FIXTURE, KEY, bar  # noqa: E402

pytestmark = pytest.mark.gpu
SCENE = os.path.join(ROOT, "tests", "golden", "tiny_scene", "blender")
ORDERS = (DO.IDENTITY, DO.PERMUTED, DO.RANDOM)


@pytest.fixture(scope="module")
def N():
    import nerf_projects_amd as N
    return N


@pytest.fixture(scope="module")
def z():
    return np.load(FIXTURE)


def tiny(N, **kw):
    return N.GridDataset.from_blender(SCENE, "train", **kw)


def small_rgb_set():
    """2 images of 7 x 5 RGB (no alpha), odd sizes that the factor 2 does not divide, poses that are no rotations."""
    rng = np.random.default_rng(7)
    images = rng.integers(0, 256, size=(2, 7, 5, 3), dtype=np.uint8)
    c2w = rng.normal(size=(2, 3, 4)).astype(np.float32)
    return images, c2w, (6.5, 7.25, 2.4, 3.6)


_CASES = {}      # name -> (dataset, the oracle's rays of the whole epoch, dirs bar, gt bar): made once, shared, never changed


def case(N, z, name):
    if name not in _CASES:
        factor = {"f1": 1, "f2": 2, "f3": 3, "f1_black": 1, "f2_black": 2, "rgb_f2": 2, "rgb_f1": 1}[name]
        white = not name.endswith("black")
        if name.startswith("rgb"):
            images, c2w, intr = small_rgb_set()
            ds = N.GridDataset.from_arrays(images, c2w, *intr, white_bkgd=white)
        else:
            ds = tiny(N, white_bkgd=white)
            images, c2w, intr = z["images_u8"], z["c2w"][:, :3, :], z["intrins_full"].tolist()
        ds.gen_rays(factor)
        rays = DO.all_rays(images, c2w, *intr, white, factor)
        _CASES[name] = (ds, rays, bar(z[f"d_dirs_{factor}"]), bar(z[f"d_gt_{factor}"]))
    return _CASES[name]


def launch(ds, order, key, begin, n):
    ds.key = key
    o, d, rgb, idx = ds._launch(order, begin, n, True)
    return o.cpu().numpy(), d.cpu().numpy(), rgb.cpu().numpy(), idx.cpu().numpy()


# ---- the kernel against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("f1", "f2", "f3", "f1_black", "f2_black", "rgb_f2", "rgb_f1"))
def test_kernel_against_oracle(N, z, name):
    ds, rays, tol_d, tol_g = case(N, z, name)
    n_rays = rays[0].shape[0]
    assert ds.n_rays == n_rays == ds.n_images * ds.h * ds.w
    worst_d = worst_g = 0.0
    for order in ORDERS:
        for n in sorted({min(v, n_rays) for v in (0, 1, 255, 256, 257)} | {n_rays}):
            begins = {0, (n_rays - n) // 3, n_rays - n}      # from the start, mid-epoch, ending at N
            if order == DO.RANDOM:
                begins.add(5 * n_rays + 3)      # draws have no end of the epoch
            for begin in sorted(begins):
                o, d, rgb, idx = launch(ds, order, KEY, begin, n)
                wo, wd, wg, widx = DO.batch(rays, order, KEY, begin, n)
                where = (name, order, begin, n)
                assert o.shape == d.shape == rgb.shape == (n, 3) and idx.shape == (n,)
                assert np.array_equal(idx, widx), where
                assert np.array_equal(o, wo), where
                if n == 0:
                    continue
                e_d, e_g = np.abs(d - wd).max(), np.abs(rgb - wg).max()
                worst_d, worst_g = max(worst_d, e_d), max(worst_g, e_g)
                assert e_d <= tol_d, where
                if ds.factor == 1:
                    assert np.array_equal(rgb, wg), where
                else:
                    assert e_g <= tol_g, where
    print(f"{name}: kernel vs oracle dirs {worst_d:.3e} (bar {tol_d:.3e}), gt {worst_g:.3e} (bar {tol_g:.3e})")


def test_another_key_is_another_epoch(N, z):
    ds, rays, _, _ = case(N, z, "f1")
    a = launch(ds, DO.PERMUTED, KEY, 0, 768)[3]
    b = launch(ds, DO.PERMUTED, KEY + 1, 0, 768)[3]
    assert np.array_equal(np.sort(a), np.arange(768)) and np.array_equal(np.sort(b), np.arange(768)) and (a != b).mean() > 0.9
    for begin in (0, 256, 512):      # the property the CPU test shows for the oracle, here for the kernel
        assert np.bincount(a[begin:begin + 256] // 256, minlength=3).min() >= 32


# ---- GridDataset ---------------------------------------------------------------------------------------------------------------
def test_from_blender_is_the_reference_s_dataset(N, z):
    ds = tiny(N)
    assert np.array_equal(ds.c2w.cpu().numpy(), z["c2w"])      # the flip and the scene scale, bit for bit
    assert np.array_equal(ds.images_u8.cpu().numpy(), z["images_u8"])
    it = ds.intrins_full
    assert [it.fx, it.fy, it.cx, it.cy] == z["intrins_full"].tolist()
    assert (ds.n_images, ds.h_full, ds.w_full, ds.h, ds.w, ds.split) == (3, 16, 16, 16, 16, "train")
    assert tuple(ds.ndc_coeffs) == (-1, -1) and ds.use_sphere_bound and ds.scene_center == [0.0] * 3 and ds.scene_radius == [1.0] * 3
    assert ds.bytes_resident == 3 * 16 * 16 * 4 + 3 * 12 * 4
    ds.gen_rays(3)
    assert (ds.h, ds.w, ds.n_rays) == (5, 5, 75) and ds.intrins.fx == it.fx * (1.0 / (16 / 5))
    assert tiny(N, n_images=2).n_rays == 512 and tiny(N, n_images=7).n_images == 3
    assert N.GridDataset.from_blender(SCENE, "test").n_images == 2


def test_batches_follow_shuffle_rays_and_epoch_size(N, z):
    _, rays, tol_d, _ = case(N, z, "f1")
    gens = [torch.Generator(device="cpu").manual_seed(11) for _ in range(2)]
    ds, twin = tiny(N, generator=gens[0]), tiny(N, generator=gens[1])
    r, gt, idx = ds.batch(100, 300, return_indices=True)      # before the first shuffle: the index order, as svox2's rays_init
    assert np.array_equal(idx.cpu().numpy(), np.arange(100, 300)) and np.array_equal(gt.cpu().numpy(), rays[2][100:300])
    ds.shuffle_rays()
    twin.shuffle_rays()
    assert ds.key == twin.key and 0 < ds.key < 2 ** 64
    first = ds.key
    r, gt, idx = ds.batch(200, 768, return_indices=True)
    wo, wd, wg, widx = DO.batch(rays, DO.PERMUTED, ds.key, 200, 568)
    assert np.array_equal(idx.cpu().numpy(), widx) and np.array_equal(gt.cpu().numpy(), wg)
    assert np.array_equal(r.origins.cpu().numpy(), wo) and np.abs(r.dirs.cpu().numpy() - wd).max() <= tol_d
    assert len(ds.batch(5, 5)[1]) == 0
    ds.shuffle_rays()
    assert ds.key != first
    test_split = N.GridDataset.from_blender(SCENE, "test")
    test_split.shuffle_rays()      # svox2 shuffles the train split only
    assert test_split.key == 0 and np.array_equal(test_split.batch(0, 9, return_indices=True)[2].cpu().numpy(), np.arange(9))
    # epoch_size: a prefix of the permutation, or that many draws
    short = tiny(N, epoch_size=300)
    assert short.n_rays == 768      # (until the first shuffle, as svox2's rays = rays_init)
    short.shuffle_rays()
    assert short.n_rays == 300 and tiny(N, epoch_size=5000).n_rays == 768
    with pytest.raises(ValueError, match="end"):
        short.batch(0, 301)
    draws = tiny(N, epoch_size=2000, permutation=False)
    draws.shuffle_rays()
    assert draws.n_rays == 2000
    idx = draws.batch(1500, 2000, return_indices=True)[2].cpu().numpy()
    assert np.array_equal(idx, DO.sigma(np.arange(1500, 2000), 768, DO.RANDOM, draws.key))


@pytest.mark.parametrize("factor", (1, 2, 3))
def test_image_and_camera_agree_with_the_batches(N, z, factor):
    ds, rays, tol_d, tol_g = case(N, z, f"f{factor}")
    hw = ds.h * ds.w
    for i in range(3):
        o, d, rgb, _ = launch(ds, DO.IDENTITY, 0, i * hw, hw)
        img = ds.image(i)
        assert tuple(img.shape) == (ds.h, ds.w, 3) and np.array_equal(img.cpu().numpy(), rgb.reshape(ds.h, ds.w, 3))
        assert np.abs(img.cpu().numpy().reshape(-1, 3) - z[f"gt_{factor}"][i * hw:(i + 1) * hw]).max() <= tol_g
        cam = ds.camera(i)
        assert (cam.width, cam.height) == (ds.w, ds.h)
        r = cam.gen_rays()
        assert np.array_equal(r.origins.cpu().numpy(), o)
        assert np.abs(r.dirs.cpu().numpy() - d).max() <= tol_d


def test_refusals(N, z):
    images, c2w, intr = small_rgb_set()
    make = N.GridDataset.from_arrays
    with pytest.raises(RuntimeError, match="images_u8"):
        make(torch.from_numpy(images), c2w, *intr)      # a CPU tensor
    with pytest.raises(TypeError, match="images_u8"):
        make(images.astype(np.float32), c2w, *intr)
    with pytest.raises(TypeError, match="images_u8"):
        make(torch.from_numpy(images).cuda().float(), c2w, *intr)
    with pytest.raises(ValueError, match="images_u8"):
        make(images[..., :2], c2w, *intr)
    with pytest.raises(ValueError, match="images_u8"):
        make(images[0], c2w, *intr)
    with pytest.raises(ValueError, match="c2w"):
        make(images, c2w[:1], *intr)
    with pytest.raises(ValueError, match="c2w"):
        make(images, c2w[:, :, :3], *intr)
    with pytest.raises(TypeError, match="c2w"):
        make(images, c2w.astype(np.int32), *intr)
    with pytest.raises(ValueError, match="fx"):
        make(images, c2w, 0.0, *intr[1:])
    with pytest.raises(ValueError, match="cy"):
        make(images, c2w, *intr[:3], float("nan"))
    with pytest.raises(ValueError, match="epoch_size"):
        make(images, c2w, *intr, epoch_size=0)
    with pytest.raises(RuntimeError, match="not a GPU"):
        make(images, c2w, *intr, device="cpu")
    ds = make(images, c2w, *intr)
    for bad in (0, 6, 2.0, True):
        with pytest.raises(ValueError, match="factor"):
            ds.gen_rays(bad)
    with pytest.raises(ValueError, match="begin"):
        ds.batch(-1, 4)
    with pytest.raises(ValueError, match="begin"):
        ds.batch(71, 70)
    with pytest.raises(ValueError, match="end"):
        ds.batch(0, 71)
    with pytest.raises(TypeError, match="end"):
        ds.batch(0, 4.0)
    with pytest.raises(TypeError, match="begin"):
        ds.batch(None, 4)
    with pytest.raises(IndexError, match="i = 2"):
        ds.image(2)
    with pytest.raises(IndexError, match="i = -1"):
        ds.camera(-1)
    assert ds.batch(0, 70)[1].shape == (70, 3)      # and nothing above has broken the dataset
    with pytest.raises(FileNotFoundError):
        N.GridDataset.from_blender(os.path.join(SCENE, "nowhere"), "train")


# ---- train_grid ------------------------------------------------------------------------------------------------------------------
def test_train_grid_on_the_tiny_scene(N):
    """40 steps of opt.py's defaults on 3 views of 16 x 16, 8^3 -> 16^3 at step 18. (The MSE condition was written without a
    GPU at hand: it states what training must do, not what a run gave.)"""
    from nerf_projects_amd.grid_fit import GridTrainConfig, evaluate, train_grid
    cfg = GridTrainConfig(reso=FT.RESO, upsamp_every=18, n_iters=40, batch_size=256)
    events = []
    ds = FT.recording_dataset(N.GridDataset, events).from_blender(SCENE, "train", generator=torch.Generator().manual_seed(3))
    test = N.GridDataset.from_blender(SCENE, "test")
    seen = []
    grid, history = train_grid(ds, cfg, test=test, generator=torch.Generator().manual_seed(5), on_eval=seen.append,
                               trainer_factory=FT.recording_trainer(N.GridTrainer, events))
    assert events == FT.expected_schedule(cfg, 768, 3)
    assert sum(e[0] == "step" for e in events) == 40 and sum(e[0] == "resample" for e in events) == 1
    assert list(grid.links.shape) == [16, 16, 16] and grid.capacity > 0 and grid.density_data.shape[0] == grid.capacity
    evals = [h for h in history if h["kind"] == "eval"]
    assert evals == seen and [e["step"] for e in evals] == list(range(0, 40, 3)) + [40]
    assert all(np.isfinite(e["mse"]) and np.isfinite(e["psnr"]) and e["n_images"] == 2 for e in evals)
    trains = [h for h in history if h["kind"] == "train"]
    assert [h["step"] for h in trains] == list(range(2, 39, 3)) + [39] and all(np.isfinite(h["mse"]) for h in trains)
    final = evaluate(grid, ds, 3)
    assert np.isfinite(final["mse"]) and np.isfinite(final["psnr"]) and final["n_images"] == 3
    start = N.SparseGrid(reso=FT.RESO[0], use_sphere_bound=True, basis_dim=9, use_z_order=True)
    start.density_data.fill_(cfg.init_sigma)
    before = evaluate(start, ds, 3)
    print(f"training-view MSE {before['mse']:.5f} -> {final['mse']:.5f}; test-view MSE {evals[0]['mse']:.5f} -> {evals[-1]['mse']:.5f}; "
          f"capacity {grid.capacity}")
    assert final["mse"] < before["mse"]
