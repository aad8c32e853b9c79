"""Sparse voxel grid at the size limits of the C ABI (include/nerf_mi355x.h, "Sparse voxel grid"), where every other test of the
grid stays small: (A) tables past 2^31 entries - the hand-made 24^3 grid of tests/test_grid_march.py at basis_dim 9 whose rows
are the LAST rows of tables of 79 536 432 + n rows, so that the first entry any kernel reads or writes is past element 2^31 of
sh_data, grad_sh, sh_rms and of a packed half table, every row below being one NaN bit pattern; (B) lattices of 2 and of 1024
nodes per axis; (C) 2^26 rays in one call. Everything is generated from seeds (tests/grid_size_edges_lib.py; the inputs are
judged on the oracle alone in tests/test_grid_size_edges_cpu.py) and compared with the numpy oracles under the bars of the
existing test of each entry. Large tables are compared on the device; only their last rows ever reach the host.
Needs a real MI355X: run with ``pytest -m gpu``."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import grid_autograd_oracle as GA
import grid_depth_autograd_oracle as DA
import grid_depth_oracle as DO
import grid_oracle as GO
import grid_regularisers_oracle as RO
import grid_size_edges_lib as L
import grid_train_losses_oracle as GL
import grid_train_oracle as GT
from test_grid import Y_MAX, cpu, gpu, make_grid, set_opt
from test_grid_autograd import assert_close
from test_grid_cpu import bar, load_fixture
from test_grid_train import assert_matches_restatement
from test_grid_train_losses_cpu import LOSSES, weights

pytestmark = pytest.mark.gpu

GIB = 1 << 30
BASIS = 9
COLS = 3 * BASIS


@pytest.fixture(scope="module")
def N():
    import nerf_projects_amd as pkg
    return pkg


def need_free(gib, what):
    """Skips when the device has less free memory than this test's peak (computed from its tensor shapes) plus 2 GiB."""
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < (gib + 2.0) * GIB:
        pytest.skip(f"{what}: needs {gib:.1f} GiB + 2 GiB of device memory, {free / GIB:.1f} GiB are free")


def states(grid):
    """the grid without skip data, then with it"""
    grid.links = grid.links      # drops the skip data
    assert not grid.accelerated
    yield False
    grid.accelerate()
    assert grid.accelerated
    yield True


def render_bar(g):
    """test_grid.py's bar of a render against the oracle at the default thresholds: the recorded bar of its fixture grid of this
    kind plus what the stop rule may drop on either side"""
    B = g["sh_data"].shape[1] // 3
    c_max = float((np.abs(g["sh_data"].reshape(-1, 3, B)) * Y_MAX[:B]).sum(-1).max() + 0.5)
    return bar(load_fixture(), "a") + 1e-7 * max(1.0, c_max)


def sample_close(got, want):
    """test_grid.py's bar of a sample: 1e-5 of the largest value (a few ulps of it)"""
    return np.abs(cpu(got) - want).max() <= 1e-5 * max(1.0, float(np.abs(want).max()))


def frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


# ========================================================================================================================
# A. tables past 2^31 entries
# ========================================================================================================================
@functools.lru_cache(maxsize=None)
def small_case():
    """the small grid as the oracles' dict, its 67 rays, a target image, 300 sample points (world), cotangents; read only"""
    g = L.hand_made_dict(BASIS)
    o, d = L.hand_made_rays()
    rng = np.random.default_rng(3)
    gt = rng.uniform(0, 1, (L.N_RAYS, 3)).astype(np.float32)
    pts = rng.uniform(-1.1, 1.1, (300, 3)).astype(np.float32)
    cot = rng.normal(size=(L.N_RAYS, 3)).astype(np.float32)
    cot_logt = rng.normal(size=(L.N_RAYS,)).astype(np.float32)
    cd, cs = rng.normal(size=(300, 1)).astype(np.float32), rng.normal(size=(300, COLS)).astype(np.float32)
    frozen(o, d, gt, pts, cot, cot_logt, cd, cs, *g.values())
    return dict(g=g, o=o, d=d, gt=gt, pts=pts, cot=cot, cot_logt=cot_logt, cd=cd, cs=cs, skip=GO.skip_distances(g["links"]),
                n=g["density_data"].shape[0])


def shifted_by_one(g):
    """The same grid with one unlinked row 0 in front of its tables: no link is 0. The edge rule of the total variation leaves
    out the cell whose own link is exactly row 0 (the reference's literal test), the one place where a result depends on WHERE
    the rows lie; a grid whose rows are the last of a large table has no such cell, and this is the small grid that has none."""
    links = np.where(g["links"] >= 0, g["links"] + 1, g["links"]).astype(np.int32)
    dens = np.concatenate([np.zeros((1, 1), np.float32), g["density_data"]])
    sh = np.concatenate([np.zeros((1, g["sh_data"].shape[1]), np.float32), g["sh_data"]])
    return dict(g, links=links, density_data=dens, sh_data=sh)


def large_table(rows_small):
    """[C, cols] float32 on the device: NaN_FILL bits in every row but the last, which are ``rows_small``"""
    n, cols = rows_small.shape
    cap = L.large_capacity(n)
    t = torch.empty((cap, cols), dtype=torch.float32, device="cuda")
    t.view(torch.int32)[:cap - n].fill_(L.NAN_FILL)
    t[cap - n:] = rows_small
    return t


def fill_is_intact(t, row0):
    """every row below ``row0`` still holds the fill pattern, bit for bit (one device reduction)"""
    return not bool((t.view(torch.int32)[:row0] != L.NAN_FILL).any())


def large_links(c):
    row0 = L.FIRST_ROW_PAST_2_31
    return gpu(np.where(c["g"]["links"] >= 0, c["g"]["links"].astype(np.int64) + row0, c["g"]["links"]).astype(np.int32))


@pytest.fixture(scope="module")
def small(N):
    c = small_case()
    grid = make_grid(N, c["g"])
    return dict(c, grid=grid, rays=N.Rays(gpu(c["o"]), gpu(c["d"])), gt_t=gpu(c["gt"]), pts_t=gpu(c["pts"]))


@pytest.fixture(scope="module")
def large(N, small):
    """The read-only large grid: sh_data is 8 GiB, density_data 0.3 GiB. No test writes into its tables."""
    need_free(8.4, "the large grid")
    links = large_links(small)
    density, sh = large_table(small["grid"].density_data), large_table(small["grid"].sh_data)
    grid = N.SparseGrid.from_tensors(links, density, sh, [1.0, 1.0, 1.0], [0.0, 0.0, 0.0])
    assert grid.capacity == L.large_capacity(small["n"]) and sh.numel() > 1 << 31
    assert int(links.max()) == grid.capacity - 1 and int(links[links >= 0].min()) == L.FIRST_ROW_PAST_2_31
    yield grid
    assert fill_is_intact(sh, L.FIRST_ROW_PAST_2_31) and fill_is_intact(density, L.FIRST_ROW_PAST_2_31)      # nobody wrote below the tail
    del grid, density, sh, links
    torch.cuda.empty_cache()


def camera_9x7(N):
    c2w = torch.tensor([[1.0, 0.0, 0.0, 0.1], [0.0, 1.0, 0.0, -0.05], [0.0, 0.0, 1.0, -2.5]])
    return N.Camera(c2w, fx=8.0, fy=8.0, cx=4.5, cy=3.5, width=9, height=7)


def forwards(N, grid, trainer, c):
    """every forward of the issue on ``grid`` as it is"""
    out = {}
    rays, pts = c["rays"], c["pts_t"]
    out["rgb"], out["logt"] = grid.volume_render(rays, return_log_transmit=True)
    out["image"] = grid.volume_render_image(camera_9x7(N))
    out["dens"], out["sh"] = grid.sample(pts)
    out["dens_alone"], _ = grid.sample(pts, want_colors=False)
    out["depth"], out["logt_depth"] = grid.volume_render_depth(rays, return_log_transmit=True)
    out["depth_thresh"] = grid.volume_render_depth(rays, sigma_thresh=5.0)
    out["rgb_taped"], out["logt_taped"] = N.GridModule(grid).volume_render(rays, return_log_transmit=True)
    assert out["rgb_taped"].requires_grad      # the taped kernel ran, not the plain one
    trainer.zero_grad()
    out["rgb_fused"] = trainer.forward_backward(rays, c["gt_t"])
    return {k: v.detach() for k, v in out.items()}


def test_large_forwards_are_the_small_grids_bit_for_bit(N, small, large):
    """Peak beside the large grid: the trainer's grad_sh and sh_rms, 2 x 8 GiB, and four [C, 1] tables."""
    need_free(16.0 + 4 * 0.3, "GridTrainer on the large grid")
    c = small
    want_rgb, want_logt = GO.render(c["g"], c["o"], c["d"])
    want_dens, want_sh = GO.sample(c["g"], c["pts"])
    tr_small, tr_large = N.GridTrainer(small["grid"]), N.GridTrainer(large)
    for (acc, _) in zip(states(small["grid"]), states(large)):
        s, b = forwards(N, small["grid"], tr_small, c), forwards(N, large, tr_large, c)
        for key in s:
            assert torch.isfinite(s[key]).all(), (key, acc)
            assert torch.equal(b[key], s[key]), (key, acc)      # (so no NaN of the fill reaches an output)
        assert b["image"].shape == (7, 9, 3) and 0.3 < float((b["image"] != 1.0).any(-1).float().mean()) < 1.0      # the ball, and past it
        # ... and they are the oracle's, under test_grid.py's rules
        err = np.abs(cpu(b["rgb"]).astype(np.float64) - want_rgb).max()
        print(f"accelerated {acc}: large render vs oracle {err:.3e} (bar {render_bar(c['g']):.3e})")
        assert err <= render_bar(c["g"])
        assert np.array_equal(cpu(b["logt"]), want_logt) and (want_logt == -1e3).sum() >= 15
        assert sample_close(b["dens"], want_dens) and sample_close(b["sh"], want_sh)
        assert torch.equal(b["dens_alone"], b["dens"])
    del tr_large
    torch.cuda.empty_cache()


# ---- 2. HalfGrid ---------------------------------------------------------------------------------------------------------
HALF_FILL = 0x7e5a      # a half NaN


def test_large_half_table_pack_unpack_and_render(N, small, large):
    """Rows [C - n, C) of a [C, 32] half table (4.7 GiB; its comparison with the fill pattern makes 2.4 GiB of bools)."""
    from nerf_projects_amd import grid_half
    need_free(4.8 + 2.4, "a [C, 32] half table")
    n, cap = small["n"], large.capacity
    row0 = cap - n
    ctx = large.ctx
    small_half = N.HalfGrid.from_grid(small["grid"])
    big = torch.empty((cap, 32), dtype=torch.float16, device="cuda")
    big.view(torch.int16).fill_(HALF_FILL)
    assert big.numel() > 1 << 31 and row0 * 32 >= 1 << 31
    clamped = torch.zeros(1, dtype=torch.int64, device="cuda")
    grid_half._pack(ctx, small["grid"].sh_data, big, row0, BASIS, clamped)
    assert int(clamped) == 0
    assert torch.equal(big[row0:].view(torch.int16), small_half.sh_half.view(torch.int16))
    assert not bool((big.view(torch.int16)[:row0] != HALF_FILL).any())      # the rows below are untouched
    assert torch.equal(grid_half._unpack(ctx, big, row0, n, BASIS), grid_half._unpack(ctx, small_half.sh_half, 0, n, BASIS))
    for lanes in ("single", "pair"):
        hs = N.HalfGrid.from_grid(small_half, lanes=lanes)
        hb = N.HalfGrid.from_tensors(large.links, large.density_data, big, [1.0, 1.0, 1.0], [0.0, 0.0, 0.0], basis_dim=BASIS,
                                     lanes=lanes)
        for (acc, _) in zip(states(hs), states(hb)):
            for got, want in zip(hb.volume_render(small["rays"], return_log_transmit=True) + hb.sample(small["pts_t"]),
                                 hs.volume_render(small["rays"], return_log_transmit=True) + hs.sample(small["pts_t"])):
                assert torch.isfinite(want).all() and torch.equal(got, want), (lanes, acc)
            assert torch.equal(hb.volume_render_image(camera_9x7(N)), hs.volume_render_image(camera_9x7(N))), (lanes, acc)
    del big, hb
    torch.cuda.empty_cache()


def test_large_half_from_grid_packs_the_whole_table(N, small, large):
    """HalfGrid.from_grid of a large grid: one pack over C x 32 slots. Its own sh_data (8 GiB), three of whose tail entries are
    beyond the largest half, and the half table (4.7 GiB)."""
    need_free(8.0 + 4.8, "a large sh_data of its own and its half table")
    n, cap = small["n"], large.capacity
    row0 = cap - n
    sh_small = small["grid"].sh_data.clone()
    sh_small[5, 3], sh_small[n - 1, 26], sh_small[n // 2, 0] = 7e4, -1e6, float("inf")
    sh_small[7, 1] = 65504.0      # the largest half itself is not clamped
    sh = large_table(sh_small)
    gs = N.SparseGrid.from_tensors(small["grid"].links, small["grid"].density_data, sh_small, [1.0, 1.0, 1.0], [0.0, 0.0, 0.0])
    gb = N.SparseGrid.from_tensors(large.links, large.density_data, sh, [1.0, 1.0, 1.0], [0.0, 0.0, 0.0])
    with pytest.warns(RuntimeWarning, match=r": 3 SH coefficient"):
        hs = N.HalfGrid.from_grid(gs)
    with pytest.warns(RuntimeWarning, match=r": 3 SH coefficient"):      # the NaN rows below the tail are not "clamped"
        hb = N.HalfGrid.from_grid(gb)
    assert hb.sh_half.shape == (cap, 32)
    assert torch.equal(hb.sh_half[row0:].view(torch.int16), hs.sh_half.view(torch.int16))
    assert float(hb.sh_half[row0 + 5, 3]) == 65504.0 and float(hb.sh_half[cap - 1].min()) == -65504.0
    for lo in (0, row0 // 2, row0 - 4096):      # below the tail: the NaN of the fill in every coefficient, zero in the pad slots
        rows = hb.sh_half[lo:lo + 4096]
        assert int(torch.isnan(rows).sum()) == 4096 * COLS and int((rows.view(torch.int16) == 0).sum()) == 4096 * (32 - COLS)
    del sh, gb, hb
    torch.cuda.empty_cache()


# ---- 3. gradients --------------------------------------------------------------------------------------------------------
def nothing_below(row0, *tables):
    return not any(bool(t[:row0].any()) for t in tables)


@pytest.mark.parametrize("losses", [False, True], ids=["mse", "beta+sparsity"])
def test_large_fused_gradients_land_in_the_tail(N, small, large, losses):
    """GridTrainer on the large grid: grad_sh and sh_rms are 2 x 8 GiB, four [C, 1] tables beside them."""
    need_free(16.0 + 4 * 0.3, "GridTrainer on the large grid")
    c, row0 = small, large.capacity - small["n"]
    lb, ls = weights(np.load(LOSSES), "a", "both") if losses else (0.0, 0.0)
    if losses:
        want = GL.fused(c["g"], c["o"], c["d"], c["gt"], beta_loss=lb / L.N_RAYS, sparsity_loss=ls, skip=c["skip"])
        plain = GT.fused(c["g"], c["o"], c["d"], c["gt"], skip=c["skip"])
        assert np.abs(want[1] - plain[1]).max() > 1e-3 * np.abs(plain[1]).max()      # the two terms are not nothing here
        want_logt, want = want[4], want[:4]
    else:
        want = GT.fused(c["g"], c["o"], c["d"], c["gt"], skip=c["skip"])
        _, want_logt = GO.render(c["g"], c["o"], c["d"])
    assert (want[3] != 0).sum() > 0.2 * c["n"]
    trainer = N.GridTrainer(large)
    assert trainer.grad_sh.numel() > 1 << 31
    for acc in states(large):
        trainer.zero_grad()
        if losses:
            rgb, logt = trainer.volume_render_fused(c["rays"], c["gt_t"], beta_loss=lb, sparsity_loss=ls, return_log_transmit=True)
        else:
            rgb, logt = trainer.forward_backward(c["rays"], c["gt_t"], return_log_transmit=True)
        assert torch.equal(rgb, large.volume_render(c["rays"])) and np.array_equal(cpu(logt), want_logt)
        got = (cpu(rgb), None, cpu(trainer.grad_density[row0:]), cpu(trainer.grad_sh[row0:]), cpu(trainer.mask[row0:]))
        differ = assert_matches_restatement(f"large fused {'losses ' if losses else ''}accelerated {acc}", got, want)
        print(f"    mask rows differing (all below the bar): {differ}")
        assert nothing_below(row0, trainer.grad_sh, trainer.grad_density, trainer.mask), acc
    del trainer
    torch.cuda.empty_cache()


def test_large_module_render_backward_lands_in_the_tail(N, small, large):
    """loss = sum(cot * rgb) + sum(cot_logt * log_transmit) through GridModule.volume_render: sh_data.grad is 8 GiB, and the
    backward holds a second table of that size while it accumulates."""
    need_free(16.0 + 2 * 0.3, "sh_data.grad of the large grid")
    c, row0 = small, large.capacity - small["n"]
    _, gd_rgb, gs_o, _ = GA.render_vjp(c["g"], c["o"], c["d"], c["cot"], skip=c["skip"])
    _, _, gd_logt = DA.depth_vjp(c["g"], c["o"], c["d"], None, c["cot_logt"], skip=c["skip"])
    gd_o = gd_rgb.astype(np.float64) + gd_logt
    # each cotangent's density gradient is held to 1e-5 of its own largest entry by the existing tests; their sum to the sum
    bar_d = 1e-5 * (float(np.abs(gd_rgb).max()) + float(np.abs(gd_logt).max()))
    assert np.abs(gd_logt).max() > 0 and np.abs(gd_rgb).max() > 0
    m = N.GridModule(large)
    for acc in states(large):
        m.zero_grad(set_to_none=True)
        rgb, logt = m.volume_render(c["rays"], return_log_transmit=True)
        ((rgb * gpu(c["cot"])).sum() + (logt * gpu(c["cot_logt"])).sum()).backward()
        gd, gs = m.density_data.grad, m.sh_data.grad
        assert gs.shape == large.sh_data.shape
        err = np.abs(cpu(gd[row0:]).astype(np.float64) - gd_o).max()
        print(f"large module accelerated {acc} d/ddensity: max {err:.3e} (bar {bar_d:.3e})")
        assert err <= bar_d
        assert_close(f"large module accelerated {acc} d/dsh", cpu(gs[row0:]), gs_o)
        assert nothing_below(row0, gs, gd), acc
        gd = gs = None
        m.zero_grad(set_to_none=True)
    del m
    torch.cuda.empty_cache()


def test_large_sample_backward_lands_in_the_tail(N, small, large):
    """sh_data.grad is 8 GiB (and the backward's own table before it is handed over)."""
    need_free(16.0 + 2 * 0.3, "sh_data.grad of the large grid")
    c, row0 = small, large.capacity - small["n"]
    gd_o, gs_o = GA.sample_backward(c["g"], c["pts"], c["cd"], c["cs"])
    m = N.GridModule(large)
    dens, sh = m.sample(c["pts_t"])
    ((dens * gpu(c["cd"])).sum() + (sh * gpu(c["cs"])).sum()).backward()
    for got, want in ((m.density_data.grad, gd_o), (m.sh_data.grad, gs_o)):
        assert np.abs(want).max() > 0
        assert np.abs(cpu(got[row0:]).astype(np.float64) - want).max() <= 1e-5 * float(np.abs(want).max())
        assert nothing_below(row0, got)
    m.zero_grad(set_to_none=True)
    del m, got
    torch.cuda.empty_cache()


# ---- 4. total variation and the optimiser -----------------------------------------------------------------------------
def test_large_tv_gradients_land_in_the_tail(N, small, large):
    """add_tv_grad("sh") over the whole lattice and over a range that wraps past the last node, without and with the edge rule,
    against the restatement on the small grid that, like the large one, has no link 0 (shifted_by_one). GridTrainer on the
    large grid: 2 x 8 GiB and four [C, 1] tables."""
    need_free(16.0 + 4 * 0.3, "GridTrainer on the large grid")
    c, row0 = small, large.capacity - small["n"]
    g1 = shifted_by_one(c["g"])
    nodes = c["g"]["links"].size
    trainer = N.GridTrainer(large)
    for start, frac in ((0, 1.0), (nodes - 700, 0.1)):
        for edge in (False, True):
            trainer.zero_grad()
            s, count = trainer.add_tv_grad("sh", scaling=0.7, sparse_frac=frac, start=start, ignore_edge=edge)
            assert (s, count) == (start, max(1, int(frac * nodes))) and (frac == 1.0 or start + count > nodes)
            want, mask = np.zeros_like(g1["sh_data"]), np.zeros(c["n"] + 1, np.uint8)
            GL.tv_grad(g1, "sh", start, count, np.float32(0.7) / np.float32(count), want, mask, ignore_edge=edge)
            assert not want[0].any() and mask[0] == 0
            tol = 1e-5 * float(np.abs(want).max())
            err = np.abs(cpu(trainer.grad_sh[row0:]).astype(np.float64) - want[1:]).max()
            print(f"large tv sh start {start} count {count} edge {edge}: max {err:.3e} (bar {tol:.3e}), rows {int(mask.sum())}")
            assert tol > 0 and err <= tol
            assert np.array_equal(cpu(trainer.mask[row0:]), mask[1:])
            assert nothing_below(row0, trainer.grad_sh, trainer.mask) and not bool(trainer.grad_density.any())
    del trainer
    torch.cuda.empty_cache()


def test_large_tv_color_value_and_backward(N, small, large):
    """GridModule.tv_color: the value is the bits of the small grid's that has no link 0 either; sh_data.grad is 8 GiB (and the
    backward's own table before it is handed over)."""
    need_free(16.0 + 0.3, "sh_data.grad of the large grid")
    c, row0 = small, large.capacity - small["n"]
    g1 = shifted_by_one(c["g"])
    v64, g64 = RO.tv_autograd64(g1, "sh")
    g32 = RO.tv_grad(g1, "sh")
    big = float(np.abs(g64).max())
    m_small, m = N.GridModule(make_grid(N, g1)), N.GridModule(large)
    v_small, v = m_small.tv_color(), m.tv_color()
    assert v.requires_grad and cpu(v).tobytes() == cpu(v_small).tobytes()
    assert abs(float(v.detach()) - float(v64)) <= 1e-6 * float(v64)
    assert cpu(m.tv_color(3, 11)).tobytes() == cpu(m_small.tv_color(3, 11)).tobytes()
    v.backward()
    got = cpu(m.sh_data.grad[row0:]).astype(np.float64)
    e64, e32 = np.abs(got - g64[1:]).max(), np.abs(got - g32[1:]).max()
    print(f"large tv_color: gradient vs fp64 autograd {e64 / big:.2e}, vs restatement {e32 / big:.2e} of the largest entry (bar 1e-5)")
    assert m.density_data.grad is None and np.isfinite(got).all() and e64 <= 1e-5 * big and e32 <= 1e-5 * big
    assert nothing_below(row0, m.sh_data.grad)
    m.zero_grad(set_to_none=True)
    del m
    torch.cuda.empty_cache()


@pytest.mark.parametrize("optim", ["rmsprop", "sgd"])
def test_large_optimiser_step_moves_the_tail_only(N, small, large, optim):
    """step() writes: tables of its own. sh_data, grad_sh, sh_rms: 3 x 8 GiB; density_data and four [C, 1] tables; the
    comparison with the fill pattern makes 2 GiB of bools."""
    need_free(24.0 + 5 * 0.3 + 2.0, "a large grid of its own with its trainer")
    c, n = small, small["n"]
    row0 = large.capacity - n
    density, sh = large_table(small["grid"].density_data), large_table(small["grid"].sh_data)
    grid = N.SparseGrid.from_tensors(large.links, density, sh, [1.0, 1.0, 1.0], [0.0, 0.0, 0.0])
    twin = N.SparseGrid.from_tensors(small["grid"].links, small["grid"].density_data.clone(), small["grid"].sh_data.clone(),
                                     [1.0, 1.0, 1.0], [0.0, 0.0, 0.0])
    trainer, tr_twin = N.GridTrainer(grid), N.GridTrainer(twin)
    trainer.forward_backward(c["rays"], c["gt_t"])
    # the float atomics leave the order of a row's sum free: the twin steps from the large trainer's own gradients
    tr_twin.grad_density.copy_(trainer.grad_density[row0:])
    tr_twin.grad_sh.copy_(trainer.grad_sh[row0:])
    tr_twin.mask.copy_(trainer.mask[row0:])
    mask = cpu(tr_twin.mask)
    assert 0.2 * n < (mask != 0).sum() < n
    lr_sigma, lr_sh, minval = 30.0, 1e-2, -0.5      # test_grid_train.py's step: the clamp is hit
    want = {}
    for key, lr, grad in (("density", lr_sigma, tr_twin.grad_density), ("sh", lr_sh, tr_twin.grad_sh)):
        data, rms = c["g"][f"{key}_data"].copy(), np.zeros_like(c["g"][f"{key}_data"])
        GT.optim_step(data, rms, cpu(grad), mask, optim, lr, 0.95, 1e-8, minval)
        want[key] = (data, rms)
    for t in (trainer, tr_twin):
        t.step(lr_sigma, lr_sh, beta=0.95, epsilon=1e-8, optim=optim, minval=minval)
    for key, data, rms, data_s, rms_s in (("density", density, trainer.density_rms, twin.density_data, tr_twin.density_rms),
                                          ("sh", sh, trainer.sh_rms, twin.sh_data, tr_twin.sh_rms)):
        # the bar of a step in test_grid_train.py: bit for bit the restatement's - and the small trainer's
        assert np.array_equal(cpu(data[row0:]), want[key][0]) and np.array_equal(cpu(rms[row0:]), want[key][1]), key
        assert torch.equal(data[row0:], data_s) and torch.equal(rms[row0:], rms_s), key
        assert (want[key][0] != c["g"][f"{key}_data"]).any()
        assert (want[key][0] == np.float32(minval)).any() or (key, optim) == ("density", "sgd")      # (lr_sigma * g is small there)
        assert fill_is_intact(data, row0) and not bool(rms[:row0].any()), key      # every row below: the fill pattern, no rms
    del trainer, grid, density, sh
    torch.cuda.empty_cache()


# ---- 5. row movers that read a large table -----------------------------------------------------------------------------
def test_large_resample_and_copy_rows_read_the_tail(N, small, large):
    """resample_grid (nerf_grid_gather) to 30^3 and remove_floaters (nerf_grid_copy_rows) read the large tables and write small
    ones: nothing beside the large grid is large."""
    from nerf_projects_amd.grid_components import remove_floaters
    from nerf_projects_amd.grid_resample import resample_grid
    new_s = resample_grid(small["grid"], 30, sigma_thresh=5.0, dilate=1, accelerate=False)
    new_b = resample_grid(large, 30, sigma_thresh=5.0, dilate=1, accelerate=False)
    assert 1000 < new_s.capacity < 30 ** 3 and torch.isfinite(new_s.sh_data).all() and bool(new_s.sh_data.any())
    for key in ("links", "density_data", "sh_data"):
        assert torch.equal(getattr(new_b, key), getattr(new_s, key)), key
    kept_s, res_s = remove_floaters(small["grid"], False)
    kept_b, res_b = remove_floaters(large, False)
    assert res_s["num_floaters"] >= 1 and res_b["num_floaters"] == res_s["num_floaters"]      # the slab is one
    assert 0 < kept_s.capacity < small["n"]
    for key in ("links", "density_data", "sh_data"):
        assert torch.equal(getattr(kept_b, key), getattr(kept_s, key)), key
    # the kept rows are the old rows, bit for bit
    old, new = small["grid"].links.flatten(), kept_s.links.flatten()
    keep = new >= 0
    assert torch.equal(kept_s.sh_data[new[keep].long()], small["grid"].sh_data[old[keep].long()])


def test_large_project_sh_writes_the_last_rows(N, small, large):
    """nerf_grid_project_sh with row0 = C - 50 into a large table of its own (8 GiB; its comparison with the fill pattern makes
    2 GiB of bools) against the projection to row 0 of a 50-row table."""
    from nerf_projects_amd import _lib
    from nerf_projects_amd.grid import sh_projection_matrix
    need_free(8.0 + 2.0, "a large sh table to project into")
    m, n_dirs, cap = 50, 16, large.capacity
    rng = np.random.default_rng(50)
    raw = gpu(rng.normal(0.0, 2.0, (m, n_dirs, 4)).astype(np.float32))
    P = gpu(sh_projection_matrix(BASIS, n_dirs)[0].astype(np.float32))
    ctx = large.ctx

    def project(table, row0):
        a = _lib.GridProjectArgs()
        a.raw, a.m, a.n_dirs, a.basis_dim = raw.data_ptr(), m, n_dirs, BASIS
        a.P, a.sh_out, a.row0 = P.data_ptr(), table.data_ptr(), row0
        a.stream = ctx.stream().value
        _lib.check(ctx.lib.nerf_grid_project_sh(ctx.handle, C.byref(a)))

    want = torch.full((m, COLS), float("nan"), device="cuda")
    project(want, 0)
    assert torch.isfinite(want).all() and bool(want.any())
    table = torch.empty((cap, COLS), dtype=torch.float32, device="cuda")
    table.view(torch.int32).fill_(L.NAN_FILL)
    project(table, cap - m)
    assert torch.equal(table[cap - m:], want) and fill_is_intact(table, cap - m)
    del table
    torch.cuda.empty_cache()


# ========================================================================================================================
# B. lattices at the axis limits: 2 and 1024 nodes
# ========================================================================================================================
@functools.lru_cache(maxsize=None)
def edge_case(reso, basis_dim):
    g = L.edge_grid(reso, basis_dim)
    o, d = L.edge_rays(g)
    pts = L.edge_points(g)
    gt = np.random.default_rng(4).uniform(0, 1, (L.EDGE_RAYS, 3)).astype(np.float32)
    frozen(o, d, pts, gt, *g.values())
    return dict(g=g, o=o, d=d, pts=pts, gt=gt, skip=GO.skip_distances(g["links"]))


EDGE = pytest.mark.parametrize("reso,basis_dim", L.EDGE_LATTICES, ids=["x".join(map(str, r)) for r, _ in L.EDGE_LATTICES])


@EDGE
def test_edge_lattice_render_and_sample_counts(N, reso, basis_dim):
    """volume_render with log_transmit, plain and accelerated, under test_grid.py's rule; count_samples equal to the oracle's
    counts without and with skip data, which is what pins accelerate() at these shapes."""
    c = edge_case(reso, basis_dim)
    grid = make_grid(N, c["g"])
    rays = N.Rays(gpu(c["o"]), gpu(c["d"]))
    want, want_logt, counts = GO.render(c["g"], c["o"], c["d"], return_counts=True)
    _, _, counts_skip = GO.render(c["g"], c["o"], c["d"], skip=c["skip"], return_counts=True)
    first = None
    for acc in states(grid):
        rgb, logt = grid.volume_render(rays, return_log_transmit=True)
        err = np.abs(cpu(rgb).astype(np.float64) - want).max()
        print(f"{reso} accelerated {acc}: render vs oracle {err:.3e} (bar {render_bar(c['g']):.3e}); samples {grid.count_samples(rays=rays)}")
        assert np.isfinite(cpu(rgb)).all() and err <= render_bar(c["g"])
        assert np.array_equal(cpu(logt), want_logt)
        first = (rgb, logt) if first is None else first
        assert torch.equal(rgb, first[0]) and torch.equal(logt, first[1])
        assert grid.count_samples(rays=rays) == (counts_skip if acc else counts)
    assert counts[1] == counts_skip[1] > 0 and (max(reso) == 2 or counts_skip[0] < counts[0])


@EDGE
def test_edge_lattice_depth(N, reso, basis_dim):
    """test_grid_depth.py's rules: the expected depth within 3x the oracle's own fp32 - fp64 distance at thresholds 0, the
    threshold depth agreeing with the fp32 oracle on 99.8 % of the rays (here: on all 96); plain and accelerated the same bits."""
    c = edge_case(reso, basis_dim)
    grid = make_grid(N, c["g"])
    rays = N.Rays(gpu(c["o"]), gpu(c["d"]))
    o32 = DO.depth(c["g"], c["o"], c["d"], sigma_thresh=0.0, stop_thresh=0.0, dtype=np.float32)
    o64 = DO.depth(c["g"], c["o"], c["d"], sigma_thresh=0.0, stop_thresh=0.0, dtype=np.float64)
    dist = float(np.abs(o32[0].astype(np.float64) - o64[0]).max())
    x = 5.0
    t32 = DO.depth(c["g"], c["o"], c["d"], threshold=x, dtype=np.float32)[0].astype(np.float64)
    first = None
    for acc in states(grid):
        set_opt(grid, 1.0, 0.5, 0.0, 0.0, 0.0)
        dep, logt = grid.volume_render_depth(rays, return_log_transmit=True)
        err = np.abs(cpu(dep).astype(np.float64) - o64[0]).max()
        print(f"{reso} accelerated {acc}: depth vs fp64 oracle {err:.3e} (bar {3 * dist:.3e}), {int((dep > 0).sum())} rays with depth")
        assert dist > 0 and np.isfinite(cpu(dep)).all() and err <= 3.0 * dist and int((dep > 0).sum()) > 20
        assert torch.equal(logt, grid.volume_render(rays, return_log_transmit=True)[1])
        set_opt(grid, 1.0, 0.5, 0.0)
        hit = grid.volume_render_depth(rays, sigma_thresh=x)
        got = cpu(hit).astype(np.float64)
        agree = float((np.abs(got - t32) <= 1e-5 * np.maximum(np.abs(got), np.abs(t32))).mean())
        assert np.isfinite(got).all() and (got >= 0).all() and agree >= 0.998 and (got > 0).sum() > 20, (acc, agree)
        first = (dep, hit) if first is None else first
        assert torch.equal(dep, first[0]) and torch.equal(hit, first[1])


@EDGE
def test_edge_lattice_sample(N, reso, basis_dim):
    """256 points in grid coordinates: inside, outside the box, exactly on the faces -0.5 and size - 0.5, exactly on nodes."""
    c = edge_case(reso, basis_dim)
    grid = make_grid(N, c["g"])
    want_d, want_s = GO.sample(c["g"], c["pts"], grid_coords=True)
    world = cpu(grid.grid2world(gpu(c["pts"])))
    want_dw, want_sw = GO.sample(c["g"], world)
    for acc in states(grid):
        dens, sh = grid.sample(gpu(c["pts"]), grid_coords=True)
        assert dens.shape == want_d.shape and sh.shape == want_s.shape and np.abs(want_d).max() > 1
        assert sample_close(dens, want_d) and sample_close(sh, want_s), acc
        assert torch.equal(grid.sample(gpu(c["pts"]), grid_coords=True, want_colors=False)[0], dens)
        dens, sh = grid.sample(gpu(world))
        assert sample_close(dens, want_dw) and sample_close(sh, want_sw), acc
    # on a node the sample is the node's own row (0 where it is empty), bit for bit
    p = c["pts"]
    on_node = (p == np.floor(p)).all(-1) & (p >= 0).all(-1) & (p <= np.array(reso) - 1).all(-1)
    dens, sh = grid.sample(gpu(p[on_node]), grid_coords=True)
    assert np.array_equal(cpu(dens), want_d[on_node]) and np.array_equal(cpu(sh), want_s[on_node])


@EDGE
def test_edge_lattice_fused_gradients(N, reso, basis_dim):
    c = edge_case(reso, basis_dim)
    grid = make_grid(N, c["g"])
    rays, gt = N.Rays(gpu(c["o"]), gpu(c["d"])), gpu(c["gt"])
    want = GT.fused(c["g"], c["o"], c["d"], c["gt"], skip=c["skip"])
    trainer = N.GridTrainer(grid)
    for acc in states(grid):
        trainer.zero_grad()
        rgb, logt = trainer.forward_backward(rays, gt, return_log_transmit=True)
        assert torch.equal(rgb, grid.volume_render(rays))
        got = (cpu(rgb), cpu(logt), cpu(trainer.grad_density), cpu(trainer.grad_sh), cpu(trainer.mask))
        differ = assert_matches_restatement(f"{reso} accelerated {acc}", got, want)
        print(f"    mask rows {int((want[3] != 0).sum())} of {len(want[3])}, differing (all below the bar): {differ}")
    assert (want[3] != 0).sum() >= 0.1 * len(want[3])


@EDGE
def test_edge_lattice_tv_gradients(N, reso, basis_dim):
    """add_tv_grad for both targets over the whole lattice from a start that wraps, the colours also with the edge rule, under
    test_grid_train.py's bar: 1e-5 of the largest entry, the mask equal."""
    c = edge_case(reso, basis_dim)
    g = c["g"]
    grid = make_grid(N, g)
    trainer = N.GridTrainer(grid)
    nodes = g["links"].size
    for target, edge in (("density", False), ("sh", False), ("sh", True)):
        trainer.zero_grad()
        start = nodes - 3
        _, count = trainer.add_tv_grad(target, scaling=0.7, sparse_frac=1.0, start=start, ignore_edge=edge)
        assert count == nodes
        table = g["density_data"] if target == "density" else g["sh_data"]
        want, mask = np.zeros_like(table), np.zeros(grid.capacity, np.uint8)
        GL.tv_grad(g, target, start, count, np.float32(0.7) / np.float32(count), want, mask, ignore_edge=edge)
        got = cpu(trainer.grad_density if target == "density" else trainer.grad_sh)
        tol = 1e-5 * float(np.abs(want).max())
        err = np.abs(got.astype(np.float64) - want).max()
        print(f"{reso} tv {target} edge {edge}: max {err:.3e} (bar {tol:.3e}), rows {int(mask.sum())}")
        assert tol > 0 and err <= tol and np.array_equal(cpu(trainer.mask), mask)
        assert not cpu(trainer.grad_sh if target == "density" else trainer.grad_density).any()


def swap_rows_0_and_1(g):
    """the same field with the rows 0 and 1 exchanged, links and tables alike"""
    links = g["links"].copy()
    links[g["links"] == 0], links[g["links"] == 1] = 1, 0
    swap = np.arange(g["density_data"].shape[0])
    swap[:2] = 1, 0
    return dict(g, links=links, density_data=g["density_data"][swap].copy(), sh_data=g["sh_data"][swap].copy())


@EDGE
def test_edge_lattice_tv_values(N, reso, basis_dim):
    """GridModule.tv and tv_color, value and backward, under test_grid_regularisers.py's bars: the value within 1e-6 of the fp64
    value, the gradient within 1e-5 of its largest entry of fp64 autograd and of the restatement. The 2 x 2 x 2 lattice has one
    cell, whose own link is row 0 here: the edge rule leaves it out, the colours' value is the constant 0 with no gradient; the
    same field with that row elsewhere has the cell counted."""
    c = edge_case(reso, basis_dim)
    variants = [c["g"]]
    if max(reso) == 2:
        assert c["g"]["links"][0, 0, 0] == 0
        variants.append(swap_rows_0_and_1(c["g"]))
    for g in variants:
        m = N.GridModule(make_grid(N, g))
        for which, target in enumerate(("density", "sh")):
            v64, g64 = RO.tv_autograd64(g, target)
            g32 = RO.tv_grad(g, target)
            big = float(np.abs(g64).max())
            m.zero_grad(set_to_none=True)
            v = m.tv() if target == "density" else m.tv_color()
            got_v = float(v.detach())
            assert v.dim() == 0 and v.requires_grad and abs(got_v - float(v64)) <= 1e-6 * float(v64), (target, got_v, float(v64))
            assert cpu(v).tobytes() == cpu(m.tv() if target == "density" else m.tv_color()).tobytes()
            v.backward()
            grads = (m.density_data.grad, m.sh_data.grad)
            assert grads[1 - which] is None
            if float(v64) == 0.0:      # the one cell is left out
                assert g is c["g"] and max(reso) == 2 and target == "sh" and got_v == 0.0
                assert grads[which] is None or not bool(grads[which].any())
                continue
            got = cpu(grads[which]).astype(np.float64)
            e64, e32 = np.abs(got - g64).max(), np.abs(got - g32).max()
            print(f"{reso} tv value {target}: {got_v:.9g} (fp64 {float(v64):.9g}); gradient vs fp64 autograd {e64 / big:.2e}, vs "
                  f"restatement {e32 / big:.2e} of the largest entry (bar 1e-5)")
            assert np.isfinite(got).all() and big > 0 and e64 <= 1e-5 * big and e32 <= 1e-5 * big


@EDGE
def test_edge_lattice_half_grid_renders_its_widened_table(N, reso, basis_dim):
    c = edge_case(reso, basis_dim)
    src = make_grid(N, c["g"])
    rays = N.Rays(gpu(c["o"]), gpu(c["d"]))
    for lanes in ("single", "pair"):
        h = src.to_half(lanes=lanes)
        widened = h.to_float()
        for (acc, _) in zip(states(h), states(widened)):
            got, want = h.volume_render(rays, return_log_transmit=True), widened.volume_render(rays, return_log_transmit=True)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (lanes, acc)
            assert torch.isfinite(got[0]).all() and bool((got[1] < 0).any())
            assert h.count_samples(rays=rays) == widened.count_samples(rays=rays)


# ========================================================================================================================
# C. the ray-count limit
# ========================================================================================================================
def test_two_to_the_26_rays_in_one_call(N, small):
    """n_rays = 2^26 in one call of volume_render and of volume_render_depth: all but the last 67 rays point away from the box.
    Origins, directions and colours are 3 x 0.75 GiB, depth and two log_transmit 0.75 GiB, and as much again for the comparisons
    and for the refused call's tensors of 2^26 + 1 rays."""
    from nerf_projects_amd import _lib
    need_free(6.0, "2^26 rays")
    n = 1 << 26
    grid = small["grid"]
    grid.opt = type(grid.opt)(background_brightness=0.25)
    o = torch.empty((n + 1, 3), device="cuda")
    d = torch.empty((n + 1, 3), device="cuda")
    o[:] = torch.tensor([0.3, -0.2, 2.5], device="cuda")
    d[:] = torch.tensor([0.1, 0.3, 1.7], device="cuda")
    o[n - L.N_RAYS:n], d[n - L.N_RAYS:n] = small["rays"].origins, small["rays"].dirs
    try:
        for acc in states(grid):
            want_rgb, want_logt = grid.volume_render(small["rays"], return_log_transmit=True)
            want_dep = grid.volume_render_depth(small["rays"])
            rgb, logt = grid.volume_render(N.Rays(o[:n], d[:n]), return_log_transmit=True)
            dep, logt_d = grid.volume_render_depth(N.Rays(o[:n], d[:n]), return_log_transmit=True)
            head = n - L.N_RAYS
            assert bool(((rgb[:head] == 0.25).all(-1) & (logt[:head] == 0) & (dep[:head] == 0) & (logt_d[:head] == 0)).all()), acc
            assert torch.equal(rgb[head:], want_rgb) and torch.equal(logt[head:], want_logt), acc
            assert torch.equal(dep[head:], want_dep) and torch.equal(logt_d[head:], want_logt), acc
            assert bool((want_logt < 0).any())
            del rgb, logt, dep, logt_d
        # one ray more is refused before anything is launched: outputs of the full size keep their sentinel
        rgb = torch.full((n + 1, 3), -7.0, device="cuda")
        dep = torch.full((n + 1,), -7.0, device="cuda")
        opt = grid.opt._to_c()
        a = _lib.GridRenderArgs()
        a.origins, a.dirs, a.n_rays, a.rgb, a.use_skip = o.data_ptr(), d.data_ptr(), n + 1, rgb.data_ptr(), 1
        a.stream = grid.ctx.stream().value
        assert grid.ctx.lib.nerf_grid_render_rays(grid._handle(), C.byref(opt), C.byref(a)) == -1
        assert b"n_rays" in grid.ctx.lib.nerf_last_error()
        b = _lib.GridDepthArgs()
        b.mode, b.origins, b.dirs, b.n_rays, b.depth, b.use_skip = _lib.NERF_GRID_DEPTH_EXPECTED, o.data_ptr(), d.data_ptr(), n + 1, dep.data_ptr(), 1
        b.stream = grid.ctx.stream().value
        assert grid.ctx.lib.nerf_grid_depth_rays(grid._handle(), C.byref(opt), C.byref(b)) == -1
        assert b"n_rays" in grid.ctx.lib.nerf_last_error()
        torch.cuda.synchronize()
        assert bool((rgb == -7.0).all()) and bool((dep == -7.0).all())
        with pytest.raises(RuntimeError, match="n_rays"):
            grid.volume_render(N.Rays(o, d))
    finally:
        grid.opt = type(grid.opt)()
        del o, d
        torch.cuda.empty_cache()
