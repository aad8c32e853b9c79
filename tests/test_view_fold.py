"""The view fold of the fp16-pair inference kernel (include/nerf_mi355x.h, nerf_set_view_fold): feature_linear folded into
views_linears.0 on the device, W_vf = W_v[:, :W] W_f and b_vf = W_v[:, :W] b_f + b_v, for the networks that are eligible.

What is asserted: sigma and everything that depends on sigma alone is bit-identical with the fold on and off; the colours
stay as close to an fp64 evaluation as test_mlp_precisions_vs_fp64 asks of the pair kernel (relative to the fp32 kernel
measured on the same inputs: rms <= 1.25x + 1e-8, max <= 2x + 1e-7); rgb_map moves by at most 2e-5, the bar oracle/parity.py
sets for the fine pass at fixed depths; eligibility is what the header says; and the fold follows the weights through
optimiser steps."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from nerf_projects_amd import synthetic
from test_hip_parity import _forward_fp64, cpu, gpu, make_net

pytestmark = pytest.mark.gpu

ARCH = dict(D=8, skips=[4], use_viewdirs=True, output_ch=4)


@pytest.fixture(scope="module")
def N():
    import nerf_projects_amd as pkg
    ctx = pkg.get_context()
    ctx.set_precision("f16x2")
    ctx.set_view_fold(True)
    ctx.precision_status(reset=True)
    yield pkg
    ctx.set_view_fold(True)
    ctx.set_precision("f16x2")
    ctx.precision_status(reset=True)


@pytest.fixture(scope="module")
def rows():
    torch.manual_seed(5)
    return torch.rand(2048, 90, device="cuda") * 2 - 1


def _errors(out, want):
    """(rms, max) of the error relative to each channel's largest |value|, as test_mlp_precisions_vs_fp64 measures it."""
    e = np.abs(out.astype(np.float64) - want) / np.abs(want).max(0)
    return np.sqrt((e ** 2).mean()), e.max()


def _three_ways(N, net, x):
    """The network's rows with the fold on, with it off, and through the fp32 kernel; and whether it is folded."""
    ctx = N.get_context()
    try:
        ctx.set_view_fold(True)
        folded = ctx.view_fold_status(net.slot)
        on = cpu(net(x))
        ctx.set_view_fold(False)
        assert not ctx.view_fold_status(net.slot)
        off = cpu(net(x))
        ctx.set_precision("f32")
        f32 = cpu(net(x))
    finally:
        ctx.set_precision("f16x2")
        ctx.set_view_fold(True)
    return on, off, f32, folded


def _assert_bars(tag, out, f32, want):
    e, ref = _errors(out, want), _errors(f32, want)
    print(f"{tag}: folded-path error rms {e[0]:.3e} max {e[1]:.3e}; fp32 kernel rms {ref[0]:.3e} max {ref[1]:.3e}")
    assert e[0] <= 1.25 * ref[0] + 1e-8, (tag, e, ref)
    assert e[1] <= 2.0 * ref[1] + 1e-7, (tag, e, ref)


def test_on_against_off(N, rows):
    """Both bench networks: rows through net(x), then the first 96 lego rays through render_rays at 64 + 128 samples."""
    sds = synthetic.synthetic_pair(0)
    nets = [make_net(N, sd) for sd in sds]
    for tag, sd, net in zip(("coarse", "fine"), sds, nets):
        on, off, f32, folded = _three_ways(N, net, rows)
        assert folded, tag
        assert np.array_equal(on[:, 3], off[:, 3]), tag                 # sigma never sees the fold
        assert not np.array_equal(on[:, :3], off[:, :3]), tag           # ... and the colours did take the other path
        want = _forward_fp64(sd, rows, 8, [4], True)
        _assert_bars(tag, on, f32, want)
    g = load_golden("render_rays_lego")
    rays = gpu(g["rays"][:96])
    q = N.make_network_query_fn(N.get_embedder(10, 0)[0], N.get_embedder(4, 0)[0])
    ctx = N.get_context()
    ret, ex = {}, {}
    try:
        for on in (True, False):
            ctx.set_view_fold(on)
            ex[on] = {}
            ret[on] = N.render_rays(rays, nets[0], q, N_samples=64, N_importance=128, network_fine=nets[1], white_bkgd=True,
                                    perturb=0., raw_noise_std=0., _extras=ex[on])
    finally:
        ctx.set_view_fold(True)
    for k in ("acc_map", "disp_map", "z_std", "acc0", "disp0"):         # functions of sigma and the depths alone
        assert np.array_equal(cpu(ret[True][k]), cpu(ret[False][k])), k
    assert np.array_equal(cpu(ex[True]["z_fine"]), cpu(ex[False]["z_fine"]))
    d = np.abs(cpu(ret[True]["rgb_map"]) - cpu(ret[False]["rgb_map"])).max()
    print(f"largest |rgb_map on - off| over 96 rays: {d:.3e}")
    assert d <= 2e-5, d


def _hostile(case):
    arch = dict(ARCH)
    if case == "W=128":
        arch["W"] = 128
        return dict(synthetic.synthetic_state_dict(41, W=128)), arch
    if case == "W=100":
        arch["W"] = 100
        return dict(synthetic.synthetic_state_dict(44, W=100)), arch
    if case == "default init":
        return dict(synthetic.default_init_state_dict(3)), arch
    sd = dict(synthetic.synthetic_state_dict(7))
    wf, wv = np.asarray(sd["feature_linear.weight"]).copy(), np.asarray(sd["views_linears.0.weight"]).copy()
    if case == "1/8 of the feature rows x2^13":        # the same function: the matching view columns x2^-13
        wf[::8] *= np.float32(2.0 ** 13)
        sd["feature_linear.bias"] = np.asarray(sd["feature_linear.bias"]).copy()
        sd["feature_linear.bias"][::8] *= np.float32(2.0 ** 13)
        wv[:, :256:8] *= np.float32(2.0 ** -13)
    elif case == "W_f x1e3, W_v[:, :W] x1e-3":
        wf *= np.float32(1e3)
        wv[:, :256] *= np.float32(1e-3)
    elif case == "gamma(dir) columns x2^-10":
        wv[:, 256:] *= np.float32(2.0 ** -10)
    else:
        raise AssertionError(case)
    sd["feature_linear.weight"], sd["views_linears.0.weight"] = wf, wv
    return sd, arch


@pytest.mark.parametrize("case", ["1/8 of the feature rows x2^13", "W_f x1e3, W_v[:, :W] x1e-3", "gamma(dir) columns x2^-10",
                                  "W=128", "W=100", "default init"])
def test_hostile_folds_against_fp64(N, rows, case):
    """Folds whose factors are far apart in size, zero padding, and the weights a training run starts from: whatever the
    network reports - folded, or not eligible - its rows keep the pair kernel's bars against fp64."""
    sd, arch = _hostile(case)
    net = make_net(N, sd, **arch)
    on, off, f32, folded = _three_ways(N, net, rows)
    print(f"{case}: folded = {int(folded)}")
    want = _forward_fp64(sd, rows, 8, [4], True)
    assert np.array_equal(on[:, 3], off[:, 3])
    if not folded:
        assert not N.get_context().view_fold_status(net.slot)
        assert np.array_equal(on, off)              # not eligible: exactly the unfolded kernel
    _assert_bars(case, on, f32, want)
    N.get_context().precision_status(reset=True)


def test_eligibility(N, rows):
    ctx = N.get_context()
    x = rows[:700]

    def scaled(changes, **kw):
        sd = dict(synthetic.synthetic_state_dict(7, **kw))
        for key, f in changes.items():
            sd[key] = (np.asarray(sd[key]) * np.float32(f)).astype(np.float32)
        return sd

    bench = [make_net(N, sd) for sd in synthetic.synthetic_pair(0)]
    assert all(ctx.view_fold_status(n.slot) for n in bench)
    # the overflow networks of test_nonfinite_values_born_inside_the_network: the reference's NaN colours come from a feature
    # vector (or a view layer) the fold never forms, so they must run unfolded
    nan_w = np.asarray(synthetic.synthetic_state_dict(7)["feature_linear.weight"]).copy()
    nan_w[17, 5] = np.nan
    not_eligible = {
        "feature": scaled({"pts_linears.7.weight": 1e10, "feature_linear.weight": 1e30}),
        "views": scaled({"feature_linear.weight": 1e20, "views_linears.0.weight": 1e20}),
        "one NaN": dict(synthetic.synthetic_state_dict(7), **{"feature_linear.weight": nan_w}),
    }
    for name, sd in not_eligible.items():
        net = make_net(N, sd)
        assert not ctx.view_fold_status(net.slot), name
        on = cpu(net(x))
        ctx.set_view_fold(False)
        try:
            off = cpu(net(x))
        finally:
            ctx.set_view_fold(True)
        assert np.array_equal(on, off, equal_nan=True), name
        if name != "one NaN":
            want = _forward_fp64(sd, x, 8, [4], True, dtype=torch.float32)
            assert np.array_equal(~np.isfinite(want), ~np.isfinite(on)), name
    # without view directions there is nothing to fold
    noview = dict(D=8, skips=[4], use_viewdirs=False, output_ch=5)
    net = make_net(N, synthetic.synthetic_state_dict(8, use_viewdirs=False, output_ch=5), **noview)
    assert not ctx.view_fold_status(net.slot)
    on = cpu(net(x))
    ctx.set_view_fold(False)
    try:
        assert not any(ctx.view_fold_status(n.slot) for n in bench)
        assert np.array_equal(cpu(net(x)), on)
    finally:
        ctx.set_view_fold(True)
    assert all(ctx.view_fold_status(n.slot) for n in bench)
    ctx.precision_status(reset=True)


def test_fold_follows_the_weights(N):
    """Two optimiser steps (64 rays, 8 + 8 samples), then the fine network's rows against fp64 of the weights read back.
    The steps move the function by far more than the bars allow: the rows computed BEFORE the steps - what a fold left
    over from the old weights would give - are shown to miss them."""
    g = load_golden("train_step")
    sd_c, sd_f = synthetic.synthetic_pair(0)
    net_c, net_f = make_net(N, sd_c), make_net(N, sd_f)
    kw = dict(network_fn=net_c, network_fine=net_f, N_samples=8, N_importance=8, white_bkgd=True, perturb=1.0,
              raw_noise_std=1.0, pytest=True, ndc=False, use_viewdirs=True, near=2., far=6.,
              network_query_fn=N.make_network_query_fn(N.get_embedder(10, 0)[0], N.get_embedder(4, 0)[0]))
    rays = g["rays"][:64]
    batch_rays, target = (gpu(rays[:, 0:3]), gpu(rays[:, 3:6])), gpu(g["target"][:64])
    torch.manual_seed(6)
    x = torch.rand(512, 90, device="cuda") * 2 - 1
    ctx = N.get_context()
    before = cpu(net_f(x))
    opt = N.Adam([net_c, net_f], lr=5e-3)
    for _ in range(2):
        N.train_on_batch(800, 800, None, batch_rays, target, opt, **kw)
    assert opt.steps == 2
    assert ctx.view_fold_status(net_f.slot) and ctx.view_fold_status(net_c.slot)
    sd = {k: cpu(v) for k, v in net_f.state_dict().items()}
    want = _forward_fp64(sd, x, 8, [4], True)
    on, off, f32, folded = _three_ways(N, net_f, x)
    assert folded
    assert np.array_equal(on[:, 3], off[:, 3])
    _assert_bars("after two steps", on, f32, want)
    stale, ref = _errors(before, want), _errors(f32, want)
    assert stale[0] > 1.25 * ref[0] + 1e-8 and stale[1] > 2.0 * ref[1] + 1e-7, (stale, ref)
    ctx.precision_status(reset=True)
