"""Occupancy-grid rendering on the GPU against the CPU oracle run with a masked network (include/nerf_mi355x.h,
"Occupancy grid"): the oracle's ``render_rays`` with a ``network_query_fn`` that zeroes ``raw`` where the numpy restatement
of the keep rule (tests/test_occupancy_cpu.py) says a sample is skipped - the mask computed from ``occ.cells()`` read back, so
both sides use the same grid. Bars are those of tests/test_hip_parity.py for the same quantities of the dense render.
Needs a real MI355X: run with ``pytest -m gpu``."""
import numpy as np
import pytest
import torch

from conftest import check_resampled, load_golden
from nerf_projects_amd import synthetic
from test_occupancy_cpu import np_cells, np_keep

pytestmark = pytest.mark.gpu

KW = dict(N_samples=64, N_importance=128, white_bkgd=True)


@pytest.fixture(scope="module", params=["f16x2", "f32"])
def N(request):
    import nerf_projects_amd as pkg
    ctx = pkg.get_context()
    ctx.set_precision(request.param)
    yield pkg
    ctx.set_precision("f16x2")


@pytest.fixture(scope="module")
def O():
    from oracle import nerf_oracle
    return nerf_oracle


def gpu(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def cpu(t):
    return t.detach().cpu().numpy()


def npd(ret):
    return {k: v.detach().cpu().numpy() for k, v in ret.items()}


@pytest.fixture(scope="module")
def nets(N, weights_pair):
    sd_c, sd_f = weights_pair
    kw = dict(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=4, skips=[4], use_viewdirs=True)
    net_c, net_f = N.NeRF(**kw).load_state_dict(sd_c), N.NeRF(**kw).load_state_dict(sd_f)
    q = N.make_network_query_fn(N.get_embedder(10, 0)[0], N.get_embedder(4, 0)[0])
    return net_c, net_f, q


@pytest.fixture(scope="module")
def onets(O, weights_pair):
    sd_c, sd_f = weights_pair
    return O.NeRF(8, 256, 63, 27, 4, (4,), True, sd_c), O.NeRF(8, 256, 63, 27, 4, (4,), True, sd_f)


def masked_query(O, occ, log):
    """make_query_fn with raw zeroed where the grid (read back from the device) skips the sample; the keep masks of the
    passes are appended to `log`."""
    cells = cpu(occ.cells())
    base = O.make_query_fn(O.get_embedder(10)[0], O.get_embedder(4)[0])

    def query(pts, viewdirs, net):
        keep = np_keep(pts, cells, occ.c1, occ.c2, occ.outside)
        log.append(keep)
        with np.errstate(invalid="ignore", over="ignore"):
            raw = base(pts, viewdirs, net)
        return np.where(keep[..., None], raw, np.float32(0)).astype(np.float32)
    return query


def _close(a, b, atol, rtol):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol)


def stagewise(N, O, nets, onets, rays, occ):
    """The masked render at the masked oracle's fine depths, with the bars of test_render_rays_lego_stagewise; raw of the
    skipped samples exactly 0; evaluated / total exactly the numpy mask's count."""
    net_c, net_f, q = nets
    log, oex, ex = [], {}, {}
    want = O.render_rays(rays, onets[0], masked_query(O, occ, log), network_fine=onets[1], retraw=True, _extras=oex, **KW)
    keep_c, keep_f = log
    occ.stats(reset=True)
    ret = N.render_rays(gpu(rays), net_c, q, network_fine=net_f, retraw=True, _extras=ex, _z_vals_fine=oex["z_fine"],
                        occupancy=occ, **KW)
    ev, tot = occ.stats()
    print(f"evaluated {ev} of {tot} points ({ev / tot:.4f}); numpy mask {keep_c.sum() + keep_f.sum()}")
    assert tot == keep_c.size + keep_f.size
    assert ev == int(keep_c.sum()) + int(keep_f.sum())
    assert np.array_equal(cpu(ex["z_coarse"]), oex["z_coarse"])
    raw = cpu(ret["raw"])
    assert (raw[~keep_f] == 0).all() and not np.signbit(raw[~keep_f]).any()
    assert np.abs(cpu(ret["rgb0"]) - want["rgb0"]).max() <= 1e-5
    assert np.abs(cpu(ret["acc0"]) - want["acc0"]).max() <= 1e-5
    _close(cpu(ex["weights_coarse"]), oex["weights_coarse"], atol=2e-6, rtol=1e-4)
    sig = max(1.0, np.abs(want["raw"]).max())
    assert np.abs(raw - want["raw"]).max() <= 5e-6 * sig
    assert np.abs(cpu(ret["rgb_map"]) - want["rgb_map"]).max() <= 2e-5
    assert np.abs(cpu(ret["acc_map"]) - want["acc_map"]).max() <= 2e-5
    _close(cpu(ret["disp_map"]), want["disp_map"], atol=1e-5, rtol=1e-4)
    return ret, want, (keep_c, keep_f)


# ---- 1. grid construction ---------------------------------------------------------------------------

def test_grid_construction(N, nets):
    net_c, net_f, _ = nets
    c1, c2, reso = (-1.5, -1.2, -1.0), (1.5, 1.3, 1.1), (33, 40, 70)      # 69 cells along z: three words, the last partial
    lat = [cpu(N.density_grid(n, c1, c2, reso)) for n in (net_c, net_f)]
    assert 0.02 < (lat[0] > 0).mean() < 0.9
    for dilate in (0, 1, 2):
        occ = N.OccupancyGrid.build([net_c, net_f], c1, c2, reso, dilate=dilate)
        want = np_cells(lat, 0.0, dilate)
        got = cpu(occ.cells())
        assert got.shape == (32, 39, 69) and got.dtype == bool
        assert np.array_equal(got, want), dilate
        assert occ.n_occupied == int(want.sum()) and abs(occ.occupied_fraction - want.mean()) < 1e-12
    one = N.OccupancyGrid.build(net_f, c1, c2, reso, threshold=0.5, dilate=0)
    assert np.array_equal(cpu(one.cells()), np_cells(lat[1:], 0.5, 0))
    mask = np.random.RandomState(3).rand(5, 9, 70) < 0.3
    rt = N.OccupancyGrid.from_mask(mask, -1.0, 1.0)
    assert np.array_equal(cpu(rt.cells()), mask) and rt.n_occupied == int(mask.sum()) and rt.reso == [6, 10, 71]
    assert np.array_equal(cpu(N.OccupancyGrid.from_mask(gpu(mask), -1.0, 1.0, outside="empty").cells()), mask)
    with pytest.raises(ValueError):
        N.OccupancyGrid.from_mask(mask, -1.0, 1.0, outside="skip")


# ---- 2. an all-occupied grid is the dense render -------------------------------------------------------

def test_all_occupied_grid_is_the_dense_render_bit_for_bit(N, nets):
    """Classify, compaction and the indexed mode with nothing skipped: every output (with retraw) equals occupancy=None bit
    for bit - under "f32" as the issue asks, and under "f16x2" too (the list is the identity, so the wavefronts are the
    dense render's). Then a chunk where nothing but the last samples is kept: those rows are the dense render's in fp32."""
    net_c, net_f, q = nets
    ctx = net_c.ctx
    K, c2w, near, far = synthetic.lego_camera(800, 800)
    packed, _ = N.pack_rays(800, 800, K, c2w=c2w, ndc=False, near=near, far=far, use_viewdirs=True, device="cuda")
    full = N.OccupancyGrid.from_mask(np.ones((4, 5, 6), bool), -1.5, 1.5)
    none = N.OccupancyGrid.from_mask(np.zeros((4, 5, 6), bool), -1.5, 1.5, outside="empty")
    before = ctx.get_precision()
    try:
        for prec in ("f32", "f16x2"):
            ctx.set_precision(prec)
            for n in (1, 31, 100, 257, 1500):       # not multiples of 32 / 128 rays (nor 1024 points per workgroup)
                rays = packed[300 * 800 + 350: 300 * 800 + 350 + n].contiguous()
                dense = N.render_rays(rays, net_c, q, network_fine=net_f, retraw=True, **KW)
                full.stats(reset=True)
                sparse = N.render_rays(rays, net_c, q, network_fine=net_f, retraw=True, occupancy=full, **KW)
                assert full.stats() == (n * (64 + 192), n * (64 + 192))
                assert set(sparse) == set(dense)
                for k in dense:
                    assert torch.equal(sparse[k], dense[k]), (prec, n, k)
                coarse = N.render_rays(rays, net_c, q, retraw=True, N_samples=64, white_bkgd=True, occupancy=full)
                dense_c = N.render_rays(rays, net_c, q, retraw=True, N_samples=64, white_bkgd=True)
                for k in dense_c:
                    assert torch.equal(coarse[k], dense_c[k]), (prec, n, k, "coarse only")
        ctx.set_precision("f32")
        rays = packed[300 * 800 + 350: 300 * 800 + 350 + 257].contiguous()
        dense_c = N.render_rays(rays, net_c, q, retraw=True, N_samples=64, white_bkgd=True)
        last = N.render_rays(rays, net_c, q, retraw=True, N_samples=64, white_bkgd=True, occupancy=none)
        assert none.stats() == (257, 257 * 64)
        assert (last["raw"][:, :-1] == 0).all() and torch.equal(last["raw"][:, -1], dense_c["raw"][:, -1])
    finally:
        ctx.set_precision(before)


# ---- 3. masked parity, stage-wise ----------------------------------------------------------------------

def test_masked_parity_stagewise(N, O, nets, onets):
    g = load_golden("render_rays_lego")
    occ = N.OccupancyGrid.build([nets[0], nets[1]], -1.5, 1.5, 65, dilate=1)
    _, _, (keep_c, keep_f) = stagewise(N, O, nets, onets, g["rays"], occ)
    assert 0 < keep_f.mean() < 1 and 0 < keep_c.mean() < 1      # the grid does skip, and does keep


# ---- 4. masked parity, free-running, on the bench frame's rays ---------------------------------------------

_BENCH_ORACLE = {}

def test_masked_parity_free_running_bench_frame(N, O, nets, onets):
    """check_resampled as test_render_rays_bench_scale uses it, the masked oracle in the reference's place. The flips are
    counted against the reference's own fp32-vs-fp64 flips on these rays (the golden's); how far the masked oracle is from
    the reference's dense render with this grid (the benchmark's) is printed first."""
    g = load_golden("bench_frame")
    net_c, net_f, q = nets
    occ = N.OccupancyGrid.build([net_c, net_f], -1.5, 1.5, 97, dilate=2)
    key = cpu(occ.cells()).tobytes()      # (the two arithmetics usually build the same cells: the oracle then runs once)
    if key not in _BENCH_ORACLE:
        oex = {}
        _BENCH_ORACLE.clear()
        _BENCH_ORACLE[key] = (O.render_rays(g["rays"], onets[0], masked_query(O, occ, []), network_fine=onets[1],
                                            _extras=oex, **KW), oex)
    want, oex = _BENCH_ORACLE[key]
    d = np.abs(want["rgb_map"] - g["rgb_map"]).max(-1)
    print(f"masked oracle vs the reference's dense render: max {d.max():.3g}, rays > 1e-4: {(d > 1e-4).sum()}")
    want = dict(want, **{k: g[k] for k in g.files if k.endswith("_fp64")})
    rays = gpu(g["rays"])
    ret = N.render_rays(rays, net_c, q, network_fine=net_f, occupancy=occ, **KW)
    for k in ("rgb0", "acc0"):
        assert np.abs(cpu(ret[k]) - want[k]).max() <= 1e-5, k
    inj = N.render_rays(rays, net_c, q, network_fine=net_f, occupancy=occ, _z_vals_fine=oex["z_fine"], **KW)
    fg = want["acc0"] > 1e-3
    st = check_resampled(npd(ret), want, injected=npd(inj), fp64=want, foreground=fg)
    print({k: v for k, v in st.items() if k != "flip_rays"})
    assert st["foreground_rays"] > 2000 and st["rgb_fg_median"] <= 2e-6 and st["rgb_fg_p99"] <= 1e-4, st


# ---- 5. adversarial masks --------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["checkerboard", "single cell", "empty grid", "box the rays leave", "coarse box, evaluate"])
def test_adversarial_masks(N, O, nets, onets, case):
    g = load_golden("render_rays_lego")
    rays = g["rays"]
    if case == "checkerboard":
        i, j, k = np.indices((24, 24, 24))
        occ = N.OccupancyGrid.from_mask((i + j + k) % 2 == 0, -1.5, 1.5)
    elif case == "single cell":
        m = np.zeros((12, 12, 40), bool)
        m[6, 6, 33] = True
        occ = N.OccupancyGrid.from_mask(m, -1.5, 1.5, outside="empty")
    elif case == "empty grid":
        occ = N.OccupancyGrid.from_mask(np.zeros((3, 3, 3), bool), -4.0, 4.0, outside="empty")
    elif case == "box the rays leave":
        occ = N.OccupancyGrid.from_mask(np.ones((7, 8, 9), bool), (-0.5, -0.4, -0.3), (0.6, 0.5, 0.4), outside="empty")
    else:
        m = np.zeros((2, 2, 2), bool)
        m[1, 0, 1] = True
        occ = N.OccupancyGrid.from_mask(m, -0.7, 0.7, outside="evaluate")
    ret, want, (keep_c, keep_f) = stagewise(N, O, nets, onets, rays, occ)
    if case == "empty grid":
        # every ray is the background plus its last sample
        assert keep_c.sum() == len(rays) and keep_f.sum() == len(rays)
        assert (cpu(ret["raw"])[:, :-1] == 0).all()
    if case == "box the rays leave":
        assert 0 < keep_f.mean() < 0.5


def test_nan_origin_comes_out_as_nan(N, O, nets, onets):
    """NaN / infinite positions count as occupied: the reference's NaN still comes out (as in the dense test)."""
    net_c, net_f, q = nets
    rays = load_golden("render_rays_lego")["rays"][:24].copy()
    rays[3, 0] = np.nan
    rays[9, 4] = np.inf
    rays[17, 9] = np.nan
    occ = N.OccupancyGrid.build([net_c, net_f], -1.5, 1.5, 33, dilate=0, outside="empty")
    ret = N.render_rays(gpu(rays), net_c, q, network_fine=net_f, occupancy=occ, **KW)
    with np.errstate(invalid="ignore", over="ignore"):
        want = O.render_rays(rays, onets[0], masked_query(O, occ, []), network_fine=onets[1], **KW)
    for k in ("rgb_map", "rgb0"):
        assert np.array_equal(np.isnan(cpu(ret[k])).any(-1), np.isnan(want[k]).any(-1)), k
        assert np.isnan(cpu(ret[k])[[3, 9]]).all(), k
    good = np.setdiff1d(np.arange(24), [3, 9, 17])
    assert np.isfinite(cpu(ret["rgb_map"])[good]).all()
    assert np.abs(cpu(ret["rgb0"])[good] - want["rgb0"][good]).max() <= 1e-5


# ---- 6. determinism ----------------------------------------------------------------------------------------

def test_sparse_render_is_deterministic(N, nets):
    net_c, net_f, q = nets
    K, c2w, near, far = synthetic.lego_camera(800, 800)
    packed, _ = N.pack_rays(800, 800, K, c2w=c2w, ndc=False, near=near, far=far, use_viewdirs=True, device="cuda")
    rays = packed[400 * 800 + 100: 400 * 800 + 100 + 3001].contiguous()
    occ = N.OccupancyGrid.build([net_c, net_f], -1.5, 1.5, 65, dilate=1)
    a = N.render_rays(rays, net_c, q, network_fine=net_f, retraw=True, occupancy=occ, **KW)
    ev = occ.stats()
    b = N.render_rays(rays, net_c, q, network_fine=net_f, retraw=True, occupancy=occ, **KW)
    assert occ.stats() == ev and 0 < ev[0] < ev[1]
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.isfinite(a["rgb_map"]).all()


# ---- 7. evaluated / total through render and render_path ---------------------------------------------------

def test_stats_of_a_small_frame(N, nets):
    net_c, net_f, q = nets
    H = W = 40
    K, c2w, near, far = synthetic.lego_camera(H, W)
    occ = N.OccupancyGrid.build([net_c, net_f], -1.5, 1.5, 49, dilate=1)
    cells = cpu(occ.cells())
    rays = N.generate_rays(H, W, K, c2w, ndc=False, near=near, far=far, use_viewdirs=True)
    ex = {}
    one = N.render_rays(rays, net_c, q, network_fine=net_f, occupancy=occ, _extras=ex, **KW)
    r = cpu(rays)
    want_ev = 0
    for z in (cpu(ex["z_coarse"]), cpu(ex["z_fine"])):
        pts = r[:, None, 0:3] + r[:, None, 3:6] * z[..., :, None]
        want_ev += int(np_keep(pts, cells, occ.c1, occ.c2, occ.outside).sum())
    total = H * W * (64 + 192)
    assert occ.stats() == (want_ev, total) and 0 < want_ev < total
    kw = dict(network_fn=net_c, network_fine=net_f, network_query_fn=q, perturb=0., raw_noise_std=0., occupancy=occ, **KW)
    cam = dict(c2w=c2w, ndc=False, near=near, far=far, use_viewdirs=True)
    rgb, _, _, _ = N.render(H, W, K, chunk=512, **cam, **kw)           # the fused frame call, four chunks (the last of 64 rays)
    assert occ.stats() == (want_ev, total)
    # fp32: a kept point's row does not depend on where in the list it stands, so the chunking does not show. (The fp16-pair
    # kernel takes its input scale per wavefront, and another chunking packs other points into a wavefront: last bits.)
    if net_c.ctx.get_precision() == "f32":
        assert torch.equal(rgb.reshape(-1, 3), one["rgb_map"])
    pose = np.concatenate([np.asarray(c2w, np.float32)[:3, :4], [[0, 0, 0, 1]]], 0).astype(np.float32)
    rgbs, _ = N.render_path([pose], (H, W, float(K[0][0])), K, 512, dict(kw, **{k: v for k, v in cam.items() if k != "c2w"}))
    assert occ.stats() == (want_ev, total)
    assert np.array_equal(rgbs[0], cpu(rgb))      # the same chunks: the same bits, in either arithmetic
    with pytest.raises(NotImplementedError):
        N.render_shard(H, W, K, 2, 0, chunk=512, **cam, **kw)
    with pytest.raises(NotImplementedError):      # a foreign network_query_fn
        N.render_rays(rays, net_c, lambda p, v, n: q(p, v, n), network_fine=net_f, occupancy=occ, **KW)
    net_c.requires_grad_(True), net_f.requires_grad_(True)
    try:
        with pytest.raises(NotImplementedError):
            N.render_rays(rays[:8].contiguous(), net_c, q, network_fine=net_f, occupancy=occ, **KW)
    finally:
        net_c.requires_grad_(False), net_f.requires_grad_(False)


# ---- 8. closeness to the dense render ------------------------------------------------------------------------

def test_closeness_to_the_dense_render(N, nets):
    """The only test about the approximation: bench network, 2 048 lego-camera rays, the benchmark's grid. Caps (the CPU
    oracle alone: 0 rays differ, evaluated / total 0.410): at most 1 % of rays differ from the dense render of the same
    build by more than 1e-4 in rgb, none by more than 1e-2, evaluated / total in [0.30, 0.50]. The caps and the oracle's
    figures are those of the CPU probe, which SKIPPED the samples outside the box: outside="empty" (the box of +-1.5 holds
    everything of this scene). With outside="evaluate" the same rays evaluate 0.63 of their points on the GPU - the rays
    run from 2 to 6 in front of a camera 4 away, so a third of every ray lies outside the box - and differ no more."""
    net_c, net_f, q = nets
    K, c2w, near, far = synthetic.lego_camera(800, 800)
    packed, _ = N.pack_rays(800, 800, K, c2w=c2w, ndc=False, near=near, far=far, use_viewdirs=True, device="cuda")
    pix = np.random.RandomState(5).randint(0, 640000, 2048)
    rays = packed[torch.from_numpy(pix).cuda()].contiguous()
    occ = N.OccupancyGrid.build([net_c, net_f], -1.5, 1.5, 97, dilate=2, outside="empty")
    dense = N.render_rays(rays, net_c, q, network_fine=net_f, **KW)
    sparse = N.render_rays(rays, net_c, q, network_fine=net_f, occupancy=occ, **KW)
    ev, tot = occ.stats()
    d = cpu((sparse["rgb_map"] - dense["rgb_map"]).abs().max(-1).values)
    print(f"precision {net_c.ctx.get_precision()}: occupied cells {occ.occupied_fraction:.4f}, evaluated / total "
          f"{ev / tot:.4f}, rays > 1e-4: {(d > 1e-4).sum()} of {len(d)}, max |d rgb| {d.max():.3g}")
    assert (d > 1e-4).mean() <= 0.01
    assert d.max() <= 1e-2
    assert 0.30 <= ev / tot <= 0.50
