"""Training with an occupancy grid (``train_on_batch(..., occupancy=occ)``, include/nerf_mi355x.h "Occupancy grid") on the
GPU: against the dense step where the grid keeps everything, against the reference's loop body with a masked network query
(tests/golden/train_occupancy.npz, made by tests/golden/make_golden_train_occupancy.py) where it does not, the noise rule,
the list's edges, other networks, the loop, determinism, ``OccupancyGrid.refresh`` and the refusals."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from nerf_projects_amd import synthetic
from test_occupancy_cpu import np_keep

pytestmark = pytest.mark.gpu

F32 = np.float32
ARCH = dict(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=4, skips=[4], use_viewdirs=True)
LR = 5e-4


@pytest.fixture(scope="module", params=["f16x2", "f32"])
def N(request):
    import nerf_projects_amd as pkg
    ctx = pkg.get_context()
    ctx.set_precision(request.param)
    yield pkg
    ctx.set_precision("f16x2")


@pytest.fixture
def N32():
    """The package in fp32 arithmetic for the properties that are stated in fp32 only; the context's mode is put back."""
    import nerf_projects_amd as pkg
    ctx = pkg.get_context()
    before = ctx.get_precision()
    ctx.set_precision("f32")
    yield pkg
    ctx.set_precision(before)


@pytest.fixture(scope="module")
def G():
    g = load_golden("train_occupancy")
    sd_c, sd_f = synthetic.synthetic_pair(0)
    assert synthetic.state_dict_digest(sd_c) == str(g["digest_c"]) and synthetic.state_dict_digest(sd_f) == str(g["digest_f"])
    return g


def gpu(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def cells_of(g, name):
    nc = int(g["reso"]) - 1
    return np.unpackbits(g[f"mask.{name}"])[:nc ** 3].reshape(nc, nc, nc).astype(bool)


def grid_of(N, g, name, outside):
    return N.OccupancyGrid.from_mask(gpu(cells_of(g, name)), float(g["c1"]), float(g["c2"]), outside=outside)


def make_net(N, sd, **arch):
    kw = dict(ARCH)
    kw.update(arch)
    return N.NeRF(**kw).load_state_dict(sd)


def pair(N, sds=None, **arch):
    sd_c, sd_f = sds if sds is not None else synthetic.synthetic_pair(0)
    return make_net(N, sd_c, **arch), (make_net(N, sd_f, **arch) if sd_f is not None else None)


def run_step(N, nets, rays, target, n_samples, n_importance, occ=None, apply_update=True, z_fine=None, **kw):
    """One train_on_batch on `nets`; everything it returns and leaves behind, as numpy."""
    net_c, net_f = nets
    opt = N.Adam([n for n in nets if n is not None], lr=LR)
    args = dict(network_fn=net_c, network_fine=net_f, N_samples=n_samples, N_importance=n_importance, white_bkgd=True,
                use_viewdirs=True, ndc=False, near=2., far=6.)
    args.update(kw)
    if occ is not None:
        args["occupancy"] = occ
    out = N.train_on_batch(800, 800, None, None, gpu(target), opt, apply_update=apply_update, _packed_rays=gpu(rays),
                           _z_vals_fine=None if z_fine is None else gpu(z_fine), **args)
    res = {k: v.detach().cpu().numpy().copy() for k, v in out.items()}
    for tag, net in (("c", net_c), ("f", net_f)):
        if net is None:
            continue
        for k, v in net.grad_dict().items():
            res[f"g_{tag}.{k}"] = v.numpy().copy()
        if apply_update:
            for k, v in net.state_dict().items():
                res[f"w_{tag}.{k}"] = v.numpy().copy()
            m, v2 = net.adam_state()
            for k in m:
                res[f"m_{tag}.{k}"], res[f"v_{tag}.{k}"] = m[k].copy(), v2[k].copy()
    return res


def assert_same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (k, np.abs(a[k].astype(np.float64) - b[k]).max())


def rays8(rays):
    return np.ascontiguousarray(rays[:, :8])


# ---- 1. all occupied is the dense step ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n_rays,sc,si", [(48, 16, 32), (37, 7, 5)])
def test_full_grid_is_the_dense_step(N, G, n_rays, sc, si):
    rays, target = G["rays"][:n_rays], G["target"][:n_rays]
    kw = dict(perturb=1.0, raw_noise_std=1.0, pytest=True)
    dense = run_step(N, pair(N), rays, target, sc, si, **kw)
    occ = grid_of(N, G, "full", "evaluate")
    sparse = run_step(N, pair(N), rays, target, sc, si, occ=occ, **kw)
    assert_same_bits(dense, sparse)
    assert occ.stats() == (n_rays * (2 * sc + si), n_rays * (2 * sc + si))


# ---- 2. / 3. parity with the masked reference --------------------------------------------------------------------------

def check_against_golden(N, g, name, res):
    # the dense tests' own bars (tests/test_hip_parity.py): losses 2e-6; gradient norms max(2e-5 coarse / 2e-4 fine, 3 x the
    # reference's fp32-fp64 gap); sampled entries five times that, relative to the tensor's largest
    print(name, "losses", float(res["img_loss"]), float(g[f"{name}.img_loss"]), float(res["img_loss0"]), float(g[f"{name}.img_loss0"]))
    assert abs(float(res["img_loss0"]) - float(g[f"{name}.img_loss0"])) <= 2e-6
    assert abs(float(res["img_loss"]) - float(g[f"{name}.img_loss"])) <= 2e-6
    assert np.abs(res["rgb"] - g[f"{name}.rgb"]).max() <= 2e-5 and np.abs(res["rgb0"] - g[f"{name}.rgb0"]).max() <= 2e-5
    worst = {}
    for tag in ("c", "f"):
        names = [str(k) for k in g[f"names_{tag}"]]
        g_off = np.concatenate([[0], np.cumsum(g[f"gsub_len_{tag}"])])
        w_off = np.concatenate([[0], np.cumsum(g[f"wsub_len_{tag}"])])
        d_w = []
        for i, k in enumerate(names):
            gr = res[f"g_{tag}.{k}"].reshape(-1)
            want_norm, want_sub = float(g[f"{name}.gnorm_{tag}"][i]), g[f"{name}.gsub_{tag}"][g_off[i]:g_off[i + 1]]
            scale = np.abs(want_sub).max() + 1e-12
            tol = 2e-5 if tag == "c" else 2e-4
            gap = float(g[f"{name}.ggap_{tag}"][i]) / scale      # (printed with a failure; the bars come from the norms' gap)
            gap_n = abs(want_norm - float(g[f"{name}.gnorm_{tag}.f64"][i])) / (want_norm + 1e-30)
            tol = max(tol, 3 * gap_n)
            elem = 5 * tol
            d_norm = abs(np.linalg.norm(gr.astype(np.float64)) - want_norm)
            d_elem = np.abs(gr[::61] - want_sub).max()
            worst[tag] = max(worst.get(tag, 0.0), d_norm / (tol * want_norm + 1e-9), d_elem / (elem * scale + 1e-9))
            assert d_norm <= tol * want_norm + 1e-9, (name, tag, k, d_norm / (want_norm + 1e-30), gap_n)
            assert d_elem <= elem * scale + 1e-9, (name, tag, k, d_elem / scale, gap)
            d_w.append(res[f"w_{tag}.{k}"].reshape(-1)[::int(g["w_stride"])].astype(np.float64) -
                       g[f"{name}.wsub_{tag}"][w_off[i]:w_off[i + 1]])
        # the parameters after the Adam step, by the criterion of the dense two-step test: no further from the reference's
        # fp32 run than 3 x what its own fp32 and fp64 runs are from each other (rms floor 1e-3 lr; entries > 0.2 lr apart)
        d_w = np.concatenate(d_w)
        rms, far = np.sqrt(np.mean(d_w ** 2)), int((np.abs(d_w) > 0.2 * LR).sum())
        assert rms <= max(3.0 * float(g[f"{name}.wgap_rms_{tag}"]), 1e-3 * LR), (name, tag, rms)
        assert far <= max(3 * int(g[f"{name}.wgap_far_{tag}"]), 3), (name, tag, far)
    print(name, "largest gradient error / bar:", worst)


@pytest.mark.parametrize("name", ["ball_eval", "ball_empty", "checker_eval", "checker_empty", "empty", "ball_empty_noise"])
def test_step_matches_the_masked_reference(N, G, name):
    occ = grid_of(N, G, str(G[f"{name}.mask"]), str(G[f"{name}.outside"]))
    res = run_step(N, pair(N), G["rays"], G["target"], int(G["n_samples"]), int(G["n_importance"]), occ=occ,
                   z_fine=G[f"{name}.z_fine"], perturb=1.0, raw_noise_std=float(G[f"{name}.noise_std"]), pytest=True)
    n = len(G["rays"])
    assert occ.stats() == (int(G[f"{name}.kept_c"]) + int(G[f"{name}.kept_f"]), n * (2 * int(G["n_samples"]) + int(G["n_importance"])))
    check_against_golden(N, G, name, res)


def test_skipped_samples_have_weight_zero_under_noise(N, G):
    """A network with black colours and sigma = -100 everywhere, white background, an empty grid, sigma noise on: the last
    sample of a ray (kept, relu(-100 + noise) = 0) has alpha 0, so rgb = 1 - sum of the weights - exactly 1 iff every
    skipped sample's weight is exactly 0 (noise on a skipped sample would make fog: relu(0 + noise) > 0)."""
    sd_c, sd_f = (dict(sd) for sd in synthetic.synthetic_pair(0))
    for sd in (sd_c, sd_f):
        sd["rgb_linear.weight"] = np.zeros_like(sd["rgb_linear.weight"])
        sd["rgb_linear.bias"] = np.full_like(sd["rgb_linear.bias"], -1e4)
        sd["alpha_linear.weight"] = np.zeros_like(sd["alpha_linear.weight"])
        sd["alpha_linear.bias"] = np.full_like(sd["alpha_linear.bias"], -100.0)
    occ = grid_of(N, G, "empty", "empty")
    res = run_step(N, pair(N, (sd_c, sd_f)), G["rays"], G["target"], 16, 32, occ=occ, apply_update=False, perturb=1.0,
                   raw_noise_std=1.0, pytest=True)
    assert (res["rgb"] == 1.0).all() and (res["rgb0"] == 1.0).all()
    assert occ.stats() == (2 * 48, 48 * 64)


# ---- 4. forward is the renderer ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,outside", [("ball", "empty"), ("checker", "evaluate")])
def test_forward_is_the_renderer_in_fp32(N32, G, name, outside):
    N = N32
    occ = grid_of(N, G, name, outside)
    nets = pair(N)
    res = run_step(N, nets, G["rays"], G["target"], 16, 32, occ=occ, apply_update=False, perturb=0.0)
    q = N.make_network_query_fn(N.get_embedder(10, 0)[0], N.get_embedder(4, 0)[0])
    ret = N.render_rays(gpu(G["rays"]), nets[0], q, N_samples=16, N_importance=32, network_fine=nets[1], white_bkgd=True,
                        occupancy=occ)
    assert np.array_equal(res["rgb"], ret["rgb_map"].cpu().numpy()) and np.array_equal(res["rgb0"], ret["rgb0"].cpu().numpy())


# ---- 5. the list's edges --------------------------------------------------------------------------------------------------

def cpu_kept(g, rays, mask, outside, z_fine, sc):
    """(coarse, fine) kept counts by np_keep: the coarse depths of perturb = 0, the given fine depths."""
    t = np.linspace(0., 1., sc, dtype=F32)
    z_c = (rays[:, 6:7] * (F32(1) - t) + rays[:, 7:8] * t).astype(F32)
    cells = cells_of(g, mask)
    n = 0
    counts = []
    for z in (z_c, z_fine):
        pts = (rays[:, None, 0:3] + (rays[:, None, 3:6] * z[..., None]).astype(F32)).astype(F32)
        counts.append(int(np_keep(pts, cells, float(g["c1"]), float(g["c2"]), outside).sum()))
    return tuple(counts)


def halves_rule(N, G, nets_fn, rays, target, occ_fn, z_fine, sc, si, **kw):
    n = len(rays)
    h = n // 2 + 1
    runs = []
    for lo, hi in ((0, n), (0, h), (h, n)):
        occ = occ_fn()
        res = run_step(N, nets_fn(), rays[lo:hi], target[lo:hi], sc, si, occ=occ, apply_update=False,
                       z_fine=None if z_fine is None else z_fine[lo:hi], perturb=0.0, **kw)
        runs.append((res, occ.stats()))
    (full, st), (a, _), (b, _) = runs
    for k in full:
        if not k.startswith("g_"):
            continue
        want = (h * a[k].astype(np.float64) + (n - h) * b[k].astype(np.float64)) / n
        scale = np.abs(full[k]).max()
        assert np.abs(full[k] - want).max() <= 1e-5 * scale + 1e-12, (k, np.abs(full[k] - want).max() / (scale + 1e-30))
    return st


@pytest.mark.parametrize("mask,outside,n_rays", [("empty", "empty", 33), ("empty", "empty", 32), ("empty", "empty", 7),
                                                 ("ball", "empty", 48), ("checker", "evaluate", 41)])
def test_list_edges_gradients_add_up_and_counts(N32, G, mask, outside, n_rays):
    """A list of 1 (mod 32), of an exact multiple of 32 and of fewer than 32 points (an empty grid keeps the last sample of
    every ray: M = the ray count in both passes), and two ragged ones: the gradients of a batch are the ray-count-weighted
    mean of those of its halves (the loss is a mean over rays), and stats() is the count np_keep gives on the CPU."""
    N = N32      # (the rule is stated in fp32: in f16x2 a wavefront's input scale depends on which points share it)
    rays, target, z_fine = G["rays"][:n_rays], G["target"][:n_rays], G["ball_empty.z_fine"][:n_rays]
    st = halves_rule(N, G, lambda: pair(N), rays, target, lambda: grid_of(N, G, mask, outside), z_fine, 16, 32)
    kc, kf = cpu_kept(G, rays, mask, outside, z_fine, 16)
    assert st == (kc + kf, n_rays * 64)
    if mask == "empty":
        assert kc == kf == n_rays
        assert {33: kf % 32 == 1, 32: kf % 32 == 0, 7: kf < 32}[n_rays]


# ---- 6. other networks ----------------------------------------------------------------------------------------------------

NOVIEWS = dict(input_ch_views=0, use_viewdirs=False, output_ch=5)
OTHER = {
    "noviews": (lambda: (synthetic.synthetic_state_dict(8, **NOVIEWS), synthetic.synthetic_state_dict(48, **NOVIEWS)), NOVIEWS),
    "shared": (lambda: (synthetic.synthetic_pair(0)[0], None), {}),
    "w128": (lambda: (synthetic.synthetic_state_dict(41, W=128), synthetic.synthetic_state_dict(44, W=128)), dict(W=128)),
}


@pytest.mark.parametrize("kind", sorted(OTHER))
def test_other_networks(N, G, kind):
    sds_fn, arch = OTHER[kind]
    views = arch.get("use_viewdirs", True)
    rays = G["rays"] if views else rays8(G["rays"])
    target = G["target"]
    nets_fn = lambda: pair(N, sds_fn(), **arch)      # noqa: E731
    kw = dict(use_viewdirs=views)
    dense = run_step(N, nets_fn(), rays, target, 16, 32, perturb=1.0, raw_noise_std=1.0, pytest=True, **kw)
    sparse = run_step(N, nets_fn(), rays, target, 16, 32, occ=grid_of(N, G, "full", "evaluate"), perturb=1.0, raw_noise_std=1.0,
                      pytest=True, **kw)
    assert_same_bits(dense, sparse)
    if N.get_context().get_precision() == "f32":
        st = halves_rule(N, G, nets_fn, rays, target, lambda: grid_of(N, G, "ball", "empty"), G["ball_empty.z_fine"], 16, 32, **kw)
        assert st == (sum(cpu_kept(G, G["rays"], "ball", "empty", G["ball_empty.z_fine"], 16)), 48 * 64)


# ---- 7. the loop ----------------------------------------------------------------------------------------------------------

def test_loop_matches_the_masked_reference(N, G):
    """20 iterations under mask (i) / outside "empty" with noise, at the bar of the dense loop test: at every iteration both
    losses within 3 x the distance between the reference's fp32 and fp64 runs so far (floor 1e-5)."""
    frame = load_golden("bench_frame")
    sd_c, sd_f = synthetic.default_init_state_dict(11), synthetic.default_init_state_dict(12)
    assert synthetic.state_dict_digest(sd_c) == str(G["loop.digest_c"]) and synthetic.state_dict_digest(sd_f) == str(G["loop.digest_f"])
    net_c, net_f = make_net(N, sd_c), make_net(N, sd_f)
    occ = grid_of(N, G, "ball", "empty")
    opt = N.Adam([net_c, net_f], lr=float(G["loop.lrate"]))
    rays, target, perm = gpu(frame["rays"]), gpu(G["loop.target"]), G["loop.perm"].astype(np.int64)
    n_rand, n_iters = int(G["loop.n_rand"]), int(G["loop.n_iters"])
    seen = {"img_loss": 0.0, "img_loss0": 0.0}
    worst = dict(seen)
    for it in range(n_iters):
        lo = (it * n_rand) % len(perm)
        sel = torch.from_numpy(perm[lo:lo + n_rand]).cuda()
        out = N.train_on_batch(800, 800, None, None, target[sel], opt, _packed_rays=rays[sel], network_fn=net_c,
                               network_fine=net_f, N_samples=16, N_importance=32, white_bkgd=True, perturb=1.0,
                               raw_noise_std=1.0, pytest=True, use_viewdirs=True, occupancy=occ)
        for name in seen:
            ref32, ref64 = float(G[f"loop.{name}"][it]), float(G[f"loop.{name}.f64"][it])
            seen[name] = max(seen[name], abs(ref32 - ref64))
            bar = max(3.0 * seen[name], 1e-5)
            err = abs(float(out[name]) - ref32)
            worst[name] = max(worst[name], err / bar)
            assert err <= bar, (it, name, float(out[name]), ref32, ref64, bar)
    print("loop: largest error / bar:", worst)
    ev, tot = occ.stats()
    assert tot == n_iters * n_rand * 64 and n_iters * n_rand * 2 <= ev < tot


# ---- 8. determinism -------------------------------------------------------------------------------------------------------

def test_same_step_twice_gives_the_same_bits(N, G):
    runs = [run_step(N, pair(N), G["rays"], G["target"], 16, 32, occ=grid_of(N, G, "checker", "empty"), perturb=1.0,
                     raw_noise_std=1.0, pytest=True) for _ in range(2)]
    assert_same_bits(*runs)


# ---- 9. refresh -----------------------------------------------------------------------------------------------------------

def test_refresh_in_place(N, G):
    nets = pair(N)
    args = dict(c1=-1.5, c2=1.5, reso=17, threshold=0.5, dilate=1, outside="empty")
    occ = N.OccupancyGrid.build(list(nets), **args)
    handle, cells0 = occ._handle, occ.cells().cpu().numpy()
    opt = N.Adam(list(nets), lr=2e-2)
    kw = dict(network_fn=nets[0], network_fine=nets[1], N_samples=16, N_importance=32, white_bkgd=True, perturb=0.0,
              use_viewdirs=True, occupancy=occ)
    for _ in range(3):
        N.train_on_batch(800, 800, None, None, gpu(G["target"]), opt, _packed_rays=gpu(G["rays"]), **kw)
    assert occ.refresh(list(nets)) is occ and occ._handle is handle
    fresh = N.OccupancyGrid.build(list(nets), **args)
    cells1 = occ.cells().cpu().numpy()
    assert np.array_equal(cells1, fresh.cells().cpu().numpy()) and occ.n_occupied == fresh.n_occupied == int(cells1.sum())
    assert not np.array_equal(cells0, cells1)      # (three steps at lr 2e-2 have moved the field)
    ev, tot = occ.stats(reset=False)
    assert tot == 3 * 48 * 64                     # the counters survived the refresh ...
    N.train_on_batch(800, 800, None, None, gpu(G["target"]), opt, _packed_rays=gpu(G["rays"]), apply_update=False, **kw)
    kw["occupancy"] = fresh
    N.train_on_batch(800, 800, None, None, gpu(G["target"]), opt, _packed_rays=gpu(G["rays"]), apply_update=False, **kw)
    ev2, tot2 = occ.stats()
    assert tot2 == 4 * 48 * 64                    # ... and go on counting, by the new cells: as the fresh grid counts
    assert (ev2 - ev, 48 * 64) == fresh.stats()


# ---- 10. errors -----------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_step_working(N, G):
    nets = pair(N)
    occ = grid_of(N, G, "ball", "empty")
    opt = N.Adam(list(nets), lr=LR)
    kw = dict(network_fn=nets[0], network_fine=nets[1], N_samples=16, N_importance=32, white_bkgd=True, perturb=0.0,
              use_viewdirs=True)
    step = lambda: float(N.train_on_batch(800, 800, None, None, gpu(G["target"]), opt, _packed_rays=gpu(G["rays"]),   # noqa: E731
                                          apply_update=False, occupancy=occ, **kw)["loss"])
    want = step()
    for bad in ("grid", np.ones((16, 16, 16), bool), 3):
        with pytest.raises(TypeError):
            N.train_on_batch(800, 800, None, None, gpu(G["target"]), opt, _packed_rays=gpu(G["rays"]), occupancy=bad, **kw)
        assert step() == want
    if torch.cuda.device_count() > 1:
        other = N.OccupancyGrid.from_mask(torch.as_tensor(cells_of(G, "ball")).to("cuda:1"), -1.5, 1.5)
        with pytest.raises(ValueError):
            N.train_on_batch(800, 800, None, None, gpu(G["target"]), opt, _packed_rays=gpu(G["rays"]), occupancy=other, **kw)
        assert step() == want
    q = N.make_network_query_fn(N.get_embedder(10, 0)[0], N.get_embedder(4, 0)[0])
    for n in nets:
        n.requires_grad_(True)
    try:
        with pytest.raises(NotImplementedError):      # the taped route
            N.render_rays(gpu(G["rays"]), nets[0], q, N_samples=16, N_importance=32, network_fine=nets[1], occupancy=occ)
    finally:
        for n in nets:
            n.requires_grad_(False)
    assert step() == want
    with pytest.raises(NotImplementedError):          # the sharded route
        N.render_shard(8, 8, np.array([[10., 0, 4], [0, 10., 4], [0, 0, 1]]), 2, 0, c2w=np.eye(4)[:3], ndc=False, near=2., far=6.,
                       use_viewdirs=True, network_fn=nets[0], network_fine=nets[1], network_query_fn=q, N_samples=16,
                       N_importance=32, occupancy=occ)
    assert step() == want
