"""The per-ray view bias (nerf_mlp_h2_fold_ray_kernel, ray_view_bias_kernel) against the folded kernel on the same weights.

A folded render of ray records with a multiple of 32 samples per ray has every wavefront on one ray: the view layer's gamma(dir)
term is formed once per ray and read from LDS instead of being encoded and multiplied per point. Nothing sigma depends on
changes, so sigma and everything derived from it are compared bit for bit; the colours differ by the rounding of that one term
and are held to the fold's own bars (2e-5 on rgb_map, 1.25 x the folded path's rms error against fp64).

MI355X, rms error of the colours against fp64 relative to each channel's largest value (new path / folded path): see
profiles/ray_view_bias_ab.md."""
import numpy as np
import pytest
import torch

import view_fold_rule as R
from nerf_projects_amd import synthetic
from test_hip_parity import _forward_fp64, cpu, gpu, make_net, npd

pytestmark = pytest.mark.gpu

LEGO = dict(white_bkgd=True, perturb=0., raw_noise_std=0.)
SIGMA_ONLY = ("acc_map", "disp_map", "z_std", "acc0", "disp0")


@pytest.fixture(scope="module")
def N():
    import nerf_projects_amd as pkg
    ctx = pkg.get_context()
    ctx.set_precision("f16x2")
    ctx.set_view_fold(True)
    ctx.set_ray_view_bias(True)
    ctx.precision_status(reset=True)
    yield pkg
    ctx.set_view_fold(True)
    ctx.set_ray_view_bias(True)
    ctx.set_precision("f16x2")
    ctx.precision_status(reset=True)


@pytest.fixture(scope="module")
def bench(N):
    """The bench pair (both folded), the query, and 10 000 rays of the lego camera at 100 x 100."""
    sds = R.bench_pair()
    nets = [make_net(N, sd) for sd in sds]
    assert all(N.get_context().view_fold_status(n.slot) for n in nets)
    q = N.make_network_query_fn(N.get_embedder(10, 0)[0], N.get_embedder(4, 0)[0])
    K, c2w, near, far = synthetic.lego_camera(100, 100)
    rays, _ = N.pack_rays(100, 100, K, c2w=c2w, ndc=False, near=near, far=far, use_viewdirs=True, device="cuda")
    return sds, nets, q, rays.contiguous()


def _new_old(ctx, fn):
    """fn() with the per-ray view bias on, then off (the folded kernel); the fold is on in both."""
    out = {}
    try:
        for on in (True, False):
            ctx.set_ray_view_bias(on)
            out[on] = fn()
    finally:
        ctx.set_ray_view_bias(True)
    return out[True], out[False]


def _embed64(x, L):
    out = [x]
    for k in range(L):
        out += [np.sin(x * 2.0 ** k), np.cos(x * 2.0 ** k)]
    return np.concatenate(out, -1)


def _fp64_raw(sd, rays, z):
    """NeRF.forward in fp64 on the points the kernel evaluates: o + d z as the kernel forms it (fp32, product and sum rounded
    separately), encoded in fp64."""
    r = cpu(rays)
    o, d, v = r[:, None, 0:3], r[:, None, 3:6], r[:, -3:]
    p = (o + (d * z[..., None]).astype(np.float32)).astype(np.float32)
    x = np.concatenate([_embed64(p.reshape(-1, 3).astype(np.float64), 10),
                        _embed64(np.repeat(v.astype(np.float64), z.shape[1], axis=0), 4)], -1)
    return _forward_fp64(sd, torch.as_tensor(x), 8, [4], True)


def _rgb_errors(raw, want):
    e = np.abs(raw.reshape(-1, 4)[:, :3].astype(np.float64) - want[:, :3]) / np.abs(want[:, :3]).max(0)
    return np.sqrt((e ** 2).mean()), e.max()


@pytest.mark.parametrize("n_rays,S", [(1, 32), (3, 32), (5, 32), (3, 64), (5, 96), (2050, 32)],
                         ids=["1x32", "3x32", "5x32", "3x64", "5x96", "three-tiles"])
def test_one_pass_against_the_folded_kernel(N, bench, n_rays, S):
    """One pass of the coarse network. 1 x 32 leaves three of the workgroup's waves behind the batch's end; 3 x 32, 5 x 32 and
    5 x 96 end inside a tile; 2050 x 32 is 65 600 points, more than two tiles for every workgroup of 256 CUs (ring wrap, the
    wave's LDS slot used again). sigma: the same bits. Colours: different bits somewhere (the path did run), rgb_map within
    2e-5, and against fp64 an rms error of at most 1.25 x the folded kernel's on the same points."""
    ctx = N.get_context()
    (sd, _), (net, _), q, all_rays = bench
    rays = all_rays[4000:4000 + n_rays].contiguous()

    def run():
        ex = {}
        ret = npd(N.render_rays(rays, net, q, N_samples=S, retraw=True, _extras=ex, **LEGO))
        return ret, cpu(ex["z_coarse"])

    (new, z), (old, z_old) = _new_old(ctx, run)
    assert np.array_equal(z, z_old)
    assert new["raw"].shape == (n_rays, S, 4) and np.isfinite(new["raw"]).all()
    assert np.array_equal(new["raw"][..., 3], old["raw"][..., 3])
    for key in ("acc_map", "disp_map"):
        assert np.array_equal(new[key], old[key]), key
    assert not np.array_equal(new["raw"][..., :3], old["raw"][..., :3])
    d = np.abs(new["rgb_map"] - old["rgb_map"]).max()
    want = _fp64_raw(sd, rays, z)
    e_new, e_old = _rgb_errors(new["raw"], want), _rgb_errors(old["raw"], want)
    print(f"{n_rays} x {S}: |rgb_map new - folded| {d:.3e}; colours vs fp64 rms / max: new {e_new[0]:.3e} / {e_new[1]:.3e}, "
          f"folded {e_old[0]:.3e} / {e_old[1]:.3e}")
    assert d <= 2e-5
    assert e_new[0] <= 1.25 * e_old[0], (e_new, e_old)
    assert ctx.precision_status(reset=True) == 0


def test_odd_sample_count_falls_back(N, bench):
    """33 samples per ray: wavefronts straddle rays, the launch is the folded kernel's - the same bits with the switch on or
    off (64 + 33 = 97 in the fine pass likewise; the coarse pass at 64 does take the new path)."""
    ctx = N.get_context()
    _, (net_c, net_f), q, all_rays = bench
    rays = all_rays[4000:4005].contiguous()
    new, old = _new_old(ctx, lambda: npd(N.render_rays(rays, net_c, q, N_samples=33, retraw=True, **LEGO)))
    for k in new:
        assert np.array_equal(new[k], old[k], equal_nan=True), k
    new, old = _new_old(ctx, lambda: npd(N.render_rays(rays, net_c, q, N_samples=64, N_importance=33, network_fine=net_f,
                                                       retraw=True, **LEGO)))
    for k in SIGMA_ONLY + ("raw",):      # the fine pass reads the coarse pass through its weights, i.e. sigma, alone
        assert np.array_equal(new[k], old[k], equal_nan=True), k
    assert not np.array_equal(new["rgb0"], old["rgb0"])


def test_indexed_rays_take_the_same_rows(N, bench):
    """Through an occupancy grid (kInputRaysIndexed) a wavefront's points lie on any rays and each lane reads its own ray's
    entries: with every cell occupied the render is the dense one bit for bit, with a checkerboard sigma and the skipped rows
    are the folded kernel's and rgb_map is within 2e-5 of it. 7 rays at 64 + 128."""
    ctx = N.get_context()
    _, (net_c, net_f), q, all_rays = bench
    rays = all_rays[4000:4007].contiguous()
    kw = dict(N_samples=64, N_importance=128, network_fine=net_f, retraw=True, **LEGO)
    dense = npd(N.render_rays(rays, net_c, q, **kw))
    full = N.OccupancyGrid.from_mask(np.ones((4, 5, 6), bool), -1.5, 1.5)
    sparse = npd(N.render_rays(rays, net_c, q, occupancy=full, **kw))
    for k in dense:
        assert np.array_equal(sparse[k], dense[k], equal_nan=True), k
    i, j, k = np.indices((24, 24, 24))
    board = N.OccupancyGrid.from_mask((i + j + k) % 2 == 0, -1.5, 1.5)
    new, old = _new_old(ctx, lambda: npd(N.render_rays(rays, net_c, q, occupancy=board, **kw)))
    assert np.array_equal(new["raw"][..., 3], old["raw"][..., 3])
    assert np.array_equal(~new["raw"].any(-1), ~old["raw"].any(-1)) and (~old["raw"].any(-1)).any()
    for key in SIGMA_ONLY:
        assert np.array_equal(new[key], old[key]), key
    d = np.abs(new["rgb_map"] - old["rgb_map"]).max()
    print(f"indexed rays: largest |rgb_map new - folded| {d:.3e}")
    assert not np.array_equal(new["raw"][..., :3], old["raw"][..., :3]) and d <= 2e-5
    assert ctx.precision_status(reset=True) == 0


def test_chunking_does_not_move_a_bit(N, bench):
    """A ray's row of the table depends on the ray and the weights alone: 100 rays at 64 + 128 rendered in chunks of 7 and of 50
    are the same bits, the colours included."""
    _, (net_c, net_f), q, all_rays = bench
    rays = all_rays[4000:4100].contiguous()
    kw = dict(network_fn=net_c, network_query_fn=q, N_samples=64, N_importance=128, network_fine=net_f, retraw=True, **LEGO)
    a, b = (npd(N.batchify_rays(rays, chunk, **kw)) for chunk in (7, 50))
    for k in ("rgb_map", "rgb0", "raw", "acc_map", "disp_map"):
        assert np.array_equal(a[k], b[k]), k
    assert N.get_context().precision_status(reset=True) == 0


def test_two_networks_two_decisions(N, bench):
    """Coarse network folded, fine one not, and the reverse, in one 64 + 128 render: the pass of the network that is not folded
    is the unfolded kernel's, bit for bit, and the other pass is the new kernel's as in a render where both are folded."""
    ctx = N.get_context()
    (sd_c, sd_f), (net_c, net_f), q, all_rays = bench
    net_cx, net_fx = make_net(N, R.unfoldable_twin(sd_c)), make_net(N, R.unfoldable_twin(sd_f))
    assert not ctx.view_fold_status(net_cx.slot) and not ctx.view_fold_status(net_fx.slot)
    rays = all_rays[4000:4096].contiguous()

    def render(c, f, fold=True):
        try:
            ctx.set_view_fold(fold)
            return npd(N.render_rays(rays, c, q, N_samples=64, N_importance=128, network_fine=f, retraw=True, **LEGO))
        finally:
            ctx.set_view_fold(True)

    coarse_pass, fine_pass = ("rgb0", "acc0", "disp0"), ("raw", "rgb_map", "acc_map", "disp_map")
    both = render(net_c, net_f)
    mixed, off = render(net_c, net_fx), render(net_c, net_fx, fold=False)
    for k in coarse_pass:
        assert np.array_equal(mixed[k], both[k]), k
    for k in fine_pass:
        assert np.array_equal(mixed[k], off[k]), k
    assert not np.array_equal(mixed["rgb0"], off["rgb0"])
    mixed, off = render(net_cx, net_f), render(net_cx, net_f, fold=False)
    for k in coarse_pass:
        assert np.array_equal(mixed[k], off[k]), k
    for k in fine_pass:
        assert np.array_equal(mixed[k], both[k]), k
    assert not np.array_equal(mixed["rgb_map"], off["rgb_map"])
    assert ctx.precision_status(reset=True) == 0


def test_nan_direction(N, bench):
    """A NaN in one ray's view direction: that ray's colours are NaN, its sigma and every other ray are what they are without
    it, as on the folded path."""
    ctx = N.get_context()
    _, (net, _), q, all_rays = bench
    rays = all_rays[4000:4003].clone()
    clean = npd(N.render_rays(rays.contiguous(), net, q, N_samples=32, retraw=True, **LEGO))
    rays[1, 9] = float("nan")
    new, old = _new_old(ctx, lambda: npd(N.render_rays(rays.contiguous(), net, q, N_samples=32, retraw=True, **LEGO)))
    assert np.isnan(new["raw"][1, :, :3]).all()
    assert np.array_equal(new["raw"][..., 3], clean["raw"][..., 3])
    assert np.array_equal(new["raw"][[0, 2]], clean["raw"][[0, 2]])
    assert np.array_equal(new["raw"][..., 3], old["raw"][..., 3]) and np.array_equal(np.isnan(new["raw"]), np.isnan(old["raw"]))
    ctx.precision_status(reset=True)


def test_follows_the_weights(N, bench):
    """Two optimiser steps, then a 64-sample pass of the fine network: the stream without the gamma(dir) chunk and the table are
    made from the new weights - sigma is the folded kernel's, the colours meet the bar against fp64 of the weights read back,
    and the colours rendered BEFORE the steps miss it."""
    from conftest import load_golden
    ctx = N.get_context()
    _, _, q, all_rays = bench
    g = load_golden("train_step")
    sd_c, sd_f = synthetic.synthetic_pair(0)
    net_c, net_f = make_net(N, sd_c), make_net(N, sd_f)
    kw = dict(network_fn=net_c, network_fine=net_f, N_samples=8, N_importance=8, white_bkgd=True, perturb=1.0,
              raw_noise_std=1.0, pytest=True, ndc=False, use_viewdirs=True, near=2., far=6., network_query_fn=q)
    rays = all_rays[4000:4005].contiguous()

    def run():
        ex = {}
        ret = npd(N.render_rays(rays, net_f, q, N_samples=64, retraw=True, _extras=ex, **LEGO))
        return ret["raw"], cpu(ex["z_coarse"])

    before, _ = run()
    tr = g["rays"][:64]
    opt = N.Adam([net_c, net_f], lr=5e-3)
    for _ in range(2):
        N.train_on_batch(800, 800, None, (gpu(tr[:, 0:3]), gpu(tr[:, 3:6])), gpu(g["target"][:64]), opt, **kw)
    assert ctx.view_fold_status(net_f.slot)
    (new, z), (old, _) = _new_old(ctx, run)
    assert np.array_equal(new[..., 3], old[..., 3]) and not np.array_equal(new[..., :3], old[..., :3])
    want = _fp64_raw({k: cpu(v) for k, v in net_f.state_dict().items()}, rays, z)
    e_new, e_old, e_stale = _rgb_errors(new, want), _rgb_errors(old, want), _rgb_errors(before, want)
    print(f"after two steps, colours vs fp64 rms: new {e_new[0]:.3e}, folded {e_old[0]:.3e}, stale {e_stale[0]:.3e}")
    assert e_new[0] <= 1.25 * e_old[0] and e_stale[0] > 1.25 * e_old[0]
    ctx.precision_status(reset=True)
