"""Sparse voxel grid training data and the training driver, the parts that need no GPU: the numpy oracle of the batch kernel
against the reference's recorded rays, the order ``sigma``, ``expon_lr`` and the configuration against the reference's
values, the C ABI of the new entry point, the generated code of the kernel, and ``train_grid``'s schedule with a recording
trainer on stand-ins for the grid and the dataset."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_dataset_oracle as DO  # noqa: E402
import grid_fit_testlib as FT  # noqa: E402
from grid_testlib import assert_structs_match_c_header, compile_kernels_to_asm  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "grid_dataset.npz")
SYN = os.path.join(ROOT, "tests", "golden", "svox2_configs", "syn.json")
KEY = 0x5EEDC0DE2024        # the key the tests fix
SIZES = (1, 2, 3, 5, 768, 4096, 4097, 1_000_003)


def bar(d_ref):
    """3x the reference's own distance from exact arithmetic, never less than 2^-24 (the project's rule)."""
    return max(3.0 * float(d_ref), 2.0 ** -24)


# ---- rays and ground truth ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", (1, 2, 3))
def test_oracle_meets_the_recorded_rays_and_gt(factor):
    z = np.load(FIXTURE)
    assert os.path.getsize(FIXTURE) < 1 << 20
    assert z["images_u8"].shape == (3, 16, 16, 4) and tuple(z[f"hw_{factor}"]) == (16 // factor, 16 // factor)
    fx, fy, cx, cy = z["intrins_full"].tolist()
    o, d, g = DO.all_rays(z["images_u8"], z["c2w"][:, :3, :], fx, fy, cx, cy, True, factor)
    assert o.dtype == d.dtype == g.dtype == np.float32
    assert np.array_equal(o, z[f"origins_{factor}"])
    e_d = np.abs(d.astype(np.float64) - z[f"dirs_{factor}"]).max()
    e_g = np.abs(g.astype(np.float64) - z[f"gt_{factor}"]).max()
    print(f"factor {factor}: oracle vs reference dirs {e_d:.3e} (bar {bar(z[f'd_dirs_{factor}']):.3e}), "
          f"gt {e_g:.3e} (bar {bar(z[f'd_gt_{factor}']):.3e})")
    assert e_d <= bar(z[f"d_dirs_{factor}"])
    if factor == 1:
        assert np.array_equal(g, z["gt_1"])
    else:
        assert e_g <= bar(z[f"d_gt_{factor}"])
    # and the fp64 evaluation of the same formulas is where the recorded distance says it is
    assert np.abs(d - z[f"dirs64_{factor}"]).max() <= 2 * bar(z[f"d_dirs_{factor}"])


def test_oracle_drops_alpha_without_white_bkgd_and_takes_rgb():
    z = np.load(FIXTURE)
    u8 = z["images_u8"]
    q = DO.composite(u8, False)
    assert np.array_equal(q, u8[..., :3].astype(np.float32) / np.float32(255))
    assert np.array_equal(DO.composite(u8[..., :3], True), q)
    assert (u8[..., 3] < 255).any() and not np.array_equal(DO.composite(u8, True), q)


# ---- the order ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_sigma_is_a_bijection_that_depends_on_the_key(n):
    p = np.arange(n, dtype=np.int64)
    s, walks = DO.sigma(p, n, DO.PERMUTED, KEY, return_walks=True)
    assert s.min() >= 0 and s.max() < n and np.array_equal(np.sort(s), p)
    # cycle walking: 2^bits < 4 n, so a walk is short on average; the largest seen over these sizes and this key is 29
    # (n = 4097 in 2^14), and the bound asserted is far above anything a 4-round network gives
    print(f"n = {n}: bits {DO.feistel_bits(n)}, mean walk {walks.mean():.2f}, largest walk {int(walks.max())}")
    assert (1 << DO.feistel_bits(n)) < 4 * max(n, 2) and DO.feistel_bits(n) % 2 == 0 and walks.max() <= 256
    if n >= 768:
        other = DO.sigma(p, n, DO.PERMUTED, KEY + 1)
        assert np.array_equal(np.sort(other), p) and (other != s).mean() > 0.9
        assert (s != p).mean() > 0.9
    # a batch is that slice of the epoch, whatever its begin
    for b, e in ((0, n), (n // 3, n - n // 5), (n - 1, n), (n, n)):
        assert np.array_equal(DO.sigma(np.arange(b, e), n, DO.PERMUTED, KEY), s[b:e])
    assert np.array_equal(DO.sigma(p, n, DO.IDENTITY, KEY), p)


def test_random_order_draws_with_replacement_inside_the_epoch():
    n = 768
    p = np.arange(5 * n, dtype=np.int64)       # positions past n are drawn too: the reference's randint branch
    r = DO.sigma(p, n, DO.RANDOM, KEY)
    assert r.min() >= 0 and r.max() < n
    assert 0.55 < len(np.unique(r[:n])) / n < 0.72            # 1 - 1 / e of the rays in n draws
    assert np.abs(np.bincount(r // 256, minlength=3) / len(r) - 1 / 3).max() < 0.03
    assert not np.array_equal(r, DO.sigma(p, n, DO.RANDOM, KEY + 1))
    big = DO.sigma(np.asarray([2 ** 40 + 5, 2 ** 40 + 6]), n, DO.RANDOM, KEY)      # the high word of the position enters
    assert not np.array_equal(big, r[5:7])


def test_every_batch_of_the_tiny_scene_sees_all_three_images():
    s = DO.sigma(np.arange(768), 768, DO.PERMUTED, KEY)
    for b in range(0, 768, 256):
        counts = np.bincount(s[b:b + 256] // 256, minlength=3)
        print("batch", b, counts)
        assert counts.min() >= 32, counts


def test_round_keys_and_hash_are_the_header_s():
    """Values worked by hand from the header's definition (Python integers), so that the oracle cannot drift with the kernel."""
    def h(v):
        v &= 0xFFFFFFFF
        v ^= v >> 16
        v = (v * 0x7FEB352D) & 0xFFFFFFFF
        v ^= v >> 15
        v = (v * 0x846CA68B) & 0xFFFFFFFF
        return v ^ (v >> 16)
    for v in (0, 1, 0xFFFFFFFF, 0x12345678):
        assert int(DO.hash32(v)) == h(v)
    key = 0xFEDCBA9876543210
    assert DO.round_keys(key) == [h(h((0x76543210 + r * 0x9E3779B9) & 0xFFFFFFFF) ^ 0xFEDCBA98) for r in range(4)]
    text = open(os.path.join(ROOT, "include", "nerf_mi355x.h")).read()
    for token in ("0x7feb352d", "0x846ca68b", "0x9e3779b9", "cycle walking"):
        assert token in text


# ---- expon_lr and the configuration -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("sigma", "sh", "short"))
def test_expon_lr_equals_the_reference(name):
    from nerf_projects_amd.grid_fit import expon_lr
    z = np.load(FIXTURE)
    lr0, lr1, delay, mult, steps = z[f"lr_{name}_args"].tolist()
    assert (delay > 0) == (name != "sh")
    for step, want in zip(z["lr_steps"].tolist(), z[f"lr_{name}"].tolist()):
        got = expon_lr(step, lr0, lr1, int(delay), mult, int(steps))
        assert abs(got - want) <= 1e-12 * abs(want), (name, step, got, want)
    assert expon_lr(-1, lr0, lr1, int(delay), mult, int(steps)) == 0.0 and expon_lr(5, 0.0, 0.0) == 0.0


def test_config_reads_syn_json_and_refuses_what_is_not_built(tmp_path):
    import json
    from nerf_projects_amd.grid_fit import GridTrainConfig
    cfg = GridTrainConfig.from_json(SYN)
    assert cfg.reso == [[256, 256, 256], [512, 512, 512]] and cfg.upsamp_every == 38400 and cfg.n_iters == 200000
    assert cfg.lr_sigma == 30.0 and cfg.lr_sh == 0.01 and cfg.lambda_tv == 1e-5 and cfg.lambda_tv_sh == 1e-3
    d = GridTrainConfig()      # opt.py's defaults
    assert (d.n_iters, d.batch_size, d.sh_dim, d.upsamp_every) == (128000, 5000, 9, 38400)
    assert (d.lr_sigma_final, d.lr_sigma_decay_steps, d.lr_sigma_delay_steps, d.lr_sigma_delay_mult) == (5e-2, 250000, 15000, 1e-2)
    assert (d.lr_sh_final, d.lr_sh_decay_steps, d.lr_sh_delay_steps, d.lr_sh_delay_mult) == (5e-6, 250000, 0, 1e-2)
    assert (d.rms_beta, d.init_sigma, d.thresh_type, d.weight_thresh, d.density_thresh) == (0.95, 0.1, "weight", 0.256, 5.0)
    assert (d.max_grid_elements, d.tv_sparsity, d.tv_sh_sparsity, d.tv_decay, d.tv_early_only) == (44_000_000, 0.01, 0.01, 1.0, 1)
    assert (d.print_every, d.eval_every, d.step_size, d.near_clip, d.background_brightness) == (20, 1, 0.5, 0.0, 1.0)
    assert (d.lambda_beta, d.lambda_sparsity, d.lr_fg_begin_step, d.upsample_density_add, d.nosphereinit) == (0.0, 0.0, 0, 0.0, False)
    for key, value in (("background_nlayers", 32), ("renderer_backend", "svox1"), ("last_sample_opaque", True),
                       ("enable_random", True), ("basis_type", "mlp"), ("basis_type", "3d_texture"),
                       ("lambda_tv_lumisphere", 1e-2), ("lambda_l2_sh", 1e-4), ("lambda_tv_basis", 1e-3)):
        path = tmp_path / f"{key}.json"
        path.write_text(json.dumps({"n_iters": 10, key: value}))
        with pytest.raises(NotImplementedError, match=key):
            GridTrainConfig.from_json(path)
        with pytest.raises(NotImplementedError, match=key):
            GridTrainConfig(**{key: value})
    path = tmp_path / "unknown.json"
    path.write_text(json.dumps({"n_iters": 10, "lr_sigmaa": 1.0}))
    with pytest.raises(ValueError, match="lr_sigmaa"):
        GridTrainConfig.from_json(path)
    path.write_text(json.dumps({"save_every": 3, "lr_sigma_bg": 1.0, "reso": 64}))      # opt.py options without effect here
    assert GridTrainConfig.from_json(path).reso == [64]


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def test_struct_matches_a_c_compile_of_the_header(tmp_path):
    seen = assert_structs_match_c_header(tmp_path, {"nerf_grid_dataset_batch_args": "GridDatasetBatchArgs"}, extra_prints=[
        'printf("order identity %d\\n", NERF_GRID_ORDER_IDENTITY);', 'printf("order permuted %d\\n", NERF_GRID_ORDER_PERMUTED);',
        'printf("order random %d\\n", NERF_GRID_ORDER_RANDOM);'])
    from nerf_projects_amd import _lib
    assert seen["order"] == {"identity": _lib.NERF_GRID_ORDER_IDENTITY, "permuted": _lib.NERF_GRID_ORDER_PERMUTED,
                             "random": _lib.NERF_GRID_ORDER_RANDOM}
    assert (DO.IDENTITY, DO.PERMUTED, DO.RANDOM) == (0, 1, 2)


def good_args(_lib):
    a = _lib.GridDatasetBatchArgs()
    a.images, a.c2w, a.origins, a.dirs, a.rgb = 0x1000, 0x1000, 0x1000, 0x1000, 0x1000
    a.n_images, a.height, a.width, a.channels = 3, 16, 16, 4
    a.fx = a.fy = 22.0
    a.cx = a.cy = 8.0
    a.factor, a.order, a.begin, a.n = 1, _lib.NERF_GRID_ORDER_PERMUTED, 0, 256
    return a


def test_the_entry_is_exported_and_refuses_bad_arguments_before_it_reads_the_context():
    import nerf_projects_amd  # noqa: F401
    from nerf_projects_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "nerf_grid_dataset_batch") and "nerf_grid_dataset_batch" in _lib.EXPORTS
    fake_ctx = C.c_void_p(0x1000)      # never dereferenced: every call below is refused, or launches nothing (n = 0)
    a = good_args(_lib)
    assert lib.nerf_grid_dataset_batch(None, C.byref(a)) == -1 and b"NULL" in lib.nerf_last_error()
    assert lib.nerf_grid_dataset_batch(fake_ctx, None) == -1 and b"NULL" in lib.nerf_last_error()
    a.struct_size -= 8
    assert lib.nerf_grid_dataset_batch(fake_ctx, C.byref(a)) == -1 and b"struct_size" in lib.nerf_last_error()
    cases = [("n_images", 0, b"n_images"), ("n_images", (1 << 20) + 1, b"n_images"), ("height", 0, b"height"),
             ("width", (1 << 15) + 1, b"width"), ("channels", 2, b"channels"), ("channels", 5, b"channels"),
             ("factor", 0, b"factor"), ("factor", 17, b"factor"), ("order", 3, b"order"), ("order", -1, b"order"),
             ("fx", 0.0, b"fx"), ("fy", float("nan"), b"fy"), ("cx", float("inf"), b"cx"), ("cy", float("nan"), b"cy"),
             ("n", -1, b"n = "), ("n", (1 << 26) + 1, b"n = "), ("begin", -1, b"begin"), ("begin", 768 - 255, b"begin"),
             ("begin", 769, b"begin"), ("images", None, b"required"), ("c2w", None, b"required"), ("origins", None, b"required"),
             ("dirs", None, b"required"), ("rgb", None, b"required"), ("images", 0x1002, b"aligned")]
    for name, value, message in cases:
        a = good_args(_lib)
        setattr(a, name, value)
        assert lib.nerf_grid_dataset_batch(fake_ctx, C.byref(a)) == -1, (name, value)
        assert message in lib.nerf_last_error(), (name, value, lib.nerf_last_error())
    a = good_args(_lib)      # the epoch shrinks with the factor: 3 * 5 * 5 rays at factor 3
    a.factor, a.begin, a.n = 3, 0, 76
    assert lib.nerf_grid_dataset_batch(fake_ctx, C.byref(a)) == -1 and b"begin" in lib.nerf_last_error()
    a = good_args(_lib)      # the random order has no end of the epoch, but begin + n stays below 2^62
    a.order, a.begin = _lib.NERF_GRID_ORDER_RANDOM, (1 << 62) - 255
    assert lib.nerf_grid_dataset_batch(fake_ctx, C.byref(a)) == -1 and b"begin" in lib.nerf_last_error()
    a = good_args(_lib)      # n = 0 is accepted and launches nothing: NULL outputs, the end of the epoch as begin
    a.begin, a.n = 768, 0
    a.origins = a.dirs = a.rgb = a.images = a.c2w = None
    assert lib.nerf_grid_dataset_batch(fake_ctx, C.byref(a)) == 0


def test_the_kernel_uses_no_scratch_no_lds_and_no_inline_assembly(tmp_path):
    text, asm, build = compile_kernels_to_asm(tmp_path, "grid_dataset_kernels.hip")
    assert "grid_dataset_kernels.hip" in build.SOURCES and "grid_dataset_api.cpp" in build.SOURCES
    assert not re.search(r"\basm\b|__asm|__shared__|atomic", re.sub(r"//[^\n]*", "", text))
    kernels = re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M)
    assert len(kernels) == 1 and "grid_dataset_batch_kernel" in kernels[0], kernels
    assert [int(s) for s in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)] == [0]
    assert [int(s) for s in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", asm)] == [0]
    assert not re.search(r"\bscratch_(load|store)|\bds_(read|write)", asm)
    vgprs = [int(v) for v in re.findall(r"\.vgpr_count:\s*(\d+)", asm)]
    print("vgprs:", vgprs)
    assert vgprs[0] <= 64      # 8 waves per SIMD: the gather's latency is hidden by waves in flight


# ---- the schedule ----------------------------------------------------------------------------------------------------------------
class StubGrid:
    """What ``train_grid`` touches of a ``SparseGrid``, on the CPU."""

    def __init__(self, made, **kw):
        from nerf_projects_amd.grid import RenderOptions
        made.append(kw)
        self.reso = kw["reso"]
        self.density_data = torch.full((4, 1), -1.0)
        self.sh_data = torch.full((4, 27), -1.0)
        self.opt = RenderOptions()
        self.seen_density = []


class StubTrainer:
    def __init__(self, grid, generator=None):
        self.grid, self.generator = grid, generator

    def zero_grad(self):
        pass

    def _render(self, rgb_gt):
        self.grid.seen_density.append(float(self.grid.density_data[0, 0]))
        return torch.full_like(rgb_gt, 0.5)

    def forward_backward(self, rays, rgb_gt):
        return self._render(rgb_gt)

    def volume_render_fused(self, rays, rgb_gt, beta_loss=0.0, sparsity_loss=0.0):
        return self._render(rgb_gt)

    def add_tv_grad(self, target, scaling, sparse_frac, ignore_edge=False):
        pass

    def step(self, lr_sigma, lr_sh, beta=0.95, optim="rmsprop"):
        pass

    def resample(self, reso, **kw):
        self.grid.reso = reso
        self.grid.density_data = torch.full((8, 1), 7.0)


class StubDataset:
    n_images, n_rays, device = 3, 768, "cpu"
    scene_center, scene_radius, use_sphere_bound = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], True

    def shuffle_rays(self):
        pass

    def batch(self, begin, end):
        from nerf_projects_amd.grid import Rays
        z = torch.zeros((end - begin, 3))
        return Rays(z, z), z

    def camera(self, i):
        return ("camera", i)


def run(**overrides):
    from nerf_projects_amd.grid_fit import GridTrainConfig, train_grid
    cfg = GridTrainConfig(reso=FT.RESO, upsamp_every=6, n_iters=14, batch_size=256, **overrides)
    events, made = [], []
    gen = torch.Generator(device="cpu")
    grid, history = train_grid(FT.recording_dataset(StubDataset, events)(), cfg, generator=gen,
                               trainer_factory=FT.recording_trainer(StubTrainer, events),
                               grid_factory=lambda **kw: StubGrid(made, **kw))
    assert made == [dict(reso=[8, 8, 8], center=[0.0, 0.0, 0.0], radius=[1.0, 1.0, 1.0], use_sphere_bound=True, basis_dim=9,
                         use_z_order=True, device="cpu")]
    assert events == FT.expected_schedule(cfg, 768, 3)
    return cfg, grid, history, events


def steps_of(events):
    """The events of every training step: split at ``batch``."""
    out = []
    for e in events:
        if e[0] == "batch":
            out.append([])
        if out and e[0] not in ("shuffle_rays", "resample"):
            out[-1].append(e)
    return out


def test_schedule_with_tv_early_only():
    from nerf_projects_amd.grid_fit import expon_lr
    cfg, grid, history, events = run()
    steps = steps_of(events)
    assert len(steps) == 14 and [s[0][1:] for s in steps[:4]] == [(0, 256), (256, 512), (512, 768), (0, 256)]
    assert sum(e[0] == "shuffle_rays" for e in events) == 5      # 3 steps per epoch, the fifth epoch is cut at n_iters
    for i, s in enumerate(steps):
        names = [e[0] for e in s]
        tv = ["add_tv_grad", "add_tv_grad"] if i < 6 else []      # TV is turned off at the first upsampling
        assert names == ["batch", "zero_grad", "forward_backward"] + tv + ["step"], (i, names)
        assert s[-1] == ("step", expon_lr(i, 30.0, 5e-2, 15000, 1e-2, 250000), expon_lr(i, 1e-2, 5e-6, 0, 1e-2, 250000), 0.95, "rmsprop")
    assert steps[0][3] == ("add_tv_grad", "density", 1e-5, 0.01, False) and steps[0][4] == ("add_tv_grad", "sh", 1e-3, 0.01, True)
    assert steps[0][-1][1] == pytest.approx(30.0 * 1e-2) and steps[0][-1][2] == pytest.approx(1e-2, rel=1e-12)      # the delayed sigma rate starts at lr * mult
    resamples = [(i, e) for i, e in enumerate(events) if e[0] == "resample"]
    assert len(resamples) == 1 and resamples[0][1] == ("resample", [16, 16, 16], 5.0, 0.256 / 16, 2, 3, 44_000_000)
    assert sum(e[0] == "batch" for e in events[:resamples[0][0]]) == 6      # after the epoch that brings the steps to upsamp_every
    assert grid.reso == [16, 16, 16] and grid.seen_density[:6] == [pytest.approx(0.1)] * 6 and grid.seen_density[6:] == [7.0] * 8
    assert float(grid.sh_data.abs().max()) == 0.0
    assert (grid.opt.step_size, grid.opt.sigma_thresh, grid.opt.stop_thresh, grid.opt.near_clip) == (0.5, 1e-8, 1e-7, 0.0)
    # the loss is read at an epoch's end (print_every = 20 is never reached): one entry per epoch, the batch MSE 0.25
    assert [(h["kind"], h["step"]) for h in history] == [("train", s) for s in (2, 5, 8, 11, 13)]
    assert all(h["mse"] == pytest.approx(0.25) for h in history)


def test_schedule_with_tv_decay_and_density_thresholding():
    cfg, grid, history, events = run(tv_early_only=0, tv_decay=0.5, thresh_type="sigma", upsample_density_add=0.25, print_every=2)
    steps = steps_of(events)
    for i, s in enumerate(steps):
        k = 1.0 if i < 6 else 0.5
        assert s[3] == ("add_tv_grad", "density", 1e-5 * k, 0.01, False) and s[4] == ("add_tv_grad", "sh", 1e-3 * k, 0.01, True)
    assert [e for e in events if e[0] == "resample"] == [("resample", [16, 16, 16], 5.0, 0.256 / 16, 2, None, 44_000_000)]
    assert grid.seen_density[6:] == [7.25] * 8
    # read every second step of an epoch and at its end
    assert [h["step"] for h in history] == [1, 2, 4, 5, 7, 8, 10, 11, 13]


def test_schedule_with_a_late_foreground():
    cfg, grid, history, events = run(lr_fg_begin_step=3, lambda_beta=1e-5)
    steps = steps_of(events)
    assert [s[-1][0] == "step" for s in steps] == [False] * 3 + [True] * 11
    assert all(s[2] == ("volume_render_fused", 256, {"beta_loss": 1e-5, "sparsity_loss": 0.0}) for s in steps)
    assert grid.seen_density[:3] == [0.0] * 3 and grid.seen_density[3:6] == [pytest.approx(0.1)] * 3


def test_train_grid_does_not_modify_its_config_and_stops_mid_epoch():
    from nerf_projects_amd.grid_fit import GridTrainConfig
    cfg, grid, history, events = run()
    assert cfg == GridTrainConfig(reso=FT.RESO, upsamp_every=6, n_iters=14, batch_size=256)
    assert [e[1:] for e in events if e[0] == "batch"][-2:] == [(0, 256), (256, 512)]
