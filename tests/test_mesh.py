"""Mesh extraction on the GPU (include/nerf_mi355x.h, "Mesh extraction"; nerf-projects_amd/mesh.py): the density lattice
against run_network and the CPU oracle, marching cubes against a numpy enumeration of the crossing edges and against the
topology of analytic surfaces, determinism, sizes, refusals, and gen_mesh's end-to-end call. Run with ``pytest -m gpu``."""
import ctypes as C

import numpy as np
import pytest
import torch

from nerf_projects_amd import synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["f16x2", "f32"])
def N(request):
    """The package with the fused MLP kernel in each of its two arithmetic modes (as tests/test_hip_parity.py::N)."""
    import nerf_projects_amd as pkg
    ctx = pkg.get_context()
    ctx.set_precision(request.param)
    yield pkg
    ctx.set_precision("f16x2")


ARCH = dict(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=4, skips=[4], use_viewdirs=True)


def make_net(N, sd, **arch):
    kw = dict(ARCH)
    kw.update(arch)
    return N.NeRF(**kw).load_state_dict(sd)


def lattice_points(c1, c2, reso):
    """gen_mesh.py:104-111."""
    return np.vstack(np.meshgrid(*(np.linspace(lo, hi, sz, dtype=np.float32) for lo, hi, sz in zip(c1, c2, reso)),
                                 indexing="ij")).reshape(3, -1).T


C1, C2, RESO = (-1.3, -0.7, -1.05), (2.1, 0.9, 1.33), (37, 20, 50)      # a non-cubic lattice with awkward bounds


def sigma_via_run_network(N, net, pts):
    q = N.make_network_query_fn(N.get_embedder(10, 0)[0], N.get_embedder(4, 0)[0])
    x = torch.as_tensor(pts).cuda()[:, None, :]
    vd = torch.nn.functional.normalize(torch.ones_like(x[:, 0]), dim=-1) if net.use_viewdirs else None
    return torch.relu(q(x, vd, net)[:, 0, 3])


def test_density_grid_bit_identical_to_run_network(N):
    """density_grid == relu(run_network(...)[..., 3]) on the same lattice materialised with np.linspace, bit for bit: the
    bench network, one without view directions (5-channel output_linear) and a 128-wide one."""
    sd_c, sd_f = synthetic.synthetic_pair(0)
    nets = [("bench_fine", make_net(N, sd_f)),
            ("noviewdirs", make_net(N, synthetic.synthetic_state_dict(8, use_viewdirs=False, output_ch=5),
                                    use_viewdirs=False, output_ch=5)),
            ("w128", make_net(N, synthetic.synthetic_state_dict(41, W=128), W=128))]
    pts = lattice_points(C1, C2, RESO)
    for tag, net in nets:
        got = N.density_grid(net, C1, C2, RESO)
        assert got.shape == RESO and got.dtype == torch.float32
        want = sigma_via_run_network(N, net, pts).reshape(RESO)
        assert torch.equal(got, want), (tag, (got - want).abs().max().item())
        assert (got > 0).any() and (got == 0).any(), tag      # the lattice crosses the density's support
    # a scalar corner / resolution is broadcast to three axes (gen_mesh.py:167-175)
    got = N.density_grid(nets[0][1], -0.9, 1.1, 33)
    want = sigma_via_run_network(N, nets[0][1], lattice_points((-0.9,) * 3, (1.1,) * 3, (33,) * 3)).reshape(33, 33, 33)
    assert torch.equal(got, want)


def _embed64(x, L):
    out = [x]
    for k in range(L):
        out += [np.sin(x * 2.0 ** k), np.cos(x * 2.0 ** k)]
    return np.concatenate(out, -1)


def _forward64(sd, x, D=8, skips=(4,)):
    sd = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items()}
    lin = lambda n, h: h @ sd[n + ".weight"].T + sd[n + ".bias"]      # noqa: E731
    h = x
    for i in range(D):
        h = np.maximum(lin(f"pts_linears.{i}", h), 0.0)
        if i in skips:
            h = np.concatenate([x, h], -1)
    return lin("alpha_linear", h)[:, 0]


def test_density_grid_vs_oracle(N):
    """Against the CPU oracle's fp32 evaluation and an fp64 one. The inputs are raw points, so the bar against fp32 is
    test_run_network_fused_matches_staged's (5e-6 x scale: the encoding's sincosf at arguments up to |x| 2^9 is part of
    it); the bar against fp64 is test_mlp_forward's."""
    from oracle import nerf_oracle as O
    sd = synthetic.synthetic_state_dict(7)
    net = make_net(N, sd)
    c1, c2, reso = (-1.2, -0.8, -1.0), (1.0, 1.3, 0.7), (9, 7, 11)
    got = N.density_grid(net, c1, c2, reso).cpu().numpy().reshape(-1)
    pts = lattice_points(c1, c2, reso)
    onet = O.NeRF(8, 256, 63, 27, 4, (4,), True, sd)
    dirs = np.tile(np.float32([0.0, 0.0, 1.0]), (pts.shape[0], 1))
    raw = O.run_network(pts[:, None, :], dirs, onet, O.get_embedder(10)[0], O.get_embedder(4)[0])
    want = np.maximum(raw[:, 0, 3], 0.0)
    want64 = np.maximum(_forward64(sd, _embed64(pts.astype(np.float64), 10)), 0.0)
    scale = max(1.0, np.abs(want).max())
    assert np.abs(got - want).max() <= 5e-6 * scale
    assert np.abs(got - want64).max() <= 4 * np.abs(want - want64).max() + 1e-6
    assert (want > 0).any()


# ---- marching cubes -------------------------------------------------------------------------------------------------

def crossing_edges(vol, iso):
    """numpy enumeration of the welded vertices: (edge keys 3 * linear_index + axis in increasing order, vertices [V, 3]
    fp32 interpolated as the header states)."""
    vol = np.asarray(vol, dtype=np.float32)
    iso = np.float32(iso)
    X, Y, Z = vol.shape
    inside = vol >= iso
    lin = np.arange(vol.size, dtype=np.int64).reshape(vol.shape)
    idx = np.stack(np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij"), -1).astype(np.float32)
    keys, verts = [], []
    for ax in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        cross = inside[lo] != inside[hi]
        a, b = vol[lo][cross], vol[hi][cross]
        with np.errstate(all="ignore"):
            t = (iso - a) / (b - a)
        t = np.where(np.isfinite(t), t, np.float32(0.5)).astype(np.float32)
        p = idx[lo][cross].copy()
        p[:, ax] = p[:, ax] + t
        keys.append(3 * lin[lo][cross] + ax)
        verts.append(p)
    keys, verts = np.concatenate(keys), np.concatenate(verts)
    order = np.argsort(keys, kind="stable")
    return keys[order], verts[order]


def test_vertices_exact():
    """Crossing edges, their order and every vertex bit for bit against the numpy enumeration, on random volumes with
    exact-iso corners, NaN and +-inf planted."""
    import nerf_projects_amd as N
    rng = np.random.default_rng(3)
    for shape, iso in (((13, 11, 17), 0.25), ((2, 2, 2), 0.0), ((5, 2, 33), -0.5), ((31, 29, 3), 1.0)):
        vol = rng.standard_normal(shape).astype(np.float32)
        flat = vol.reshape(-1)
        pick = rng.permutation(flat.size)
        n = max(1, flat.size // 20)
        flat[pick[:n]] = np.float32(iso)
        flat[pick[n:2 * n]] = np.nan
        flat[pick[2 * n:3 * n]] = np.inf
        flat[pick[3 * n:4 * n]] = -np.inf
        keys, want = crossing_edges(vol, iso)
        v, t = N.marching_cubes_volume(torch.as_tensor(vol).cuda(), iso)
        got = v.cpu().numpy()
        assert got.shape == want.shape, shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), shape
        tri = t.cpu().numpy()
        assert tri.dtype == np.int64 and (tri.size == 0 or (tri.min() >= 0 and tri.max() < len(want)))
        _check_cells(tri, keys, shape)


def _check_cells(tri, keys, shape):
    """Every triangle's three edges belong to one cell."""
    X, Y, Z = shape
    p, ax = keys // 3, keys % 3
    ijk = np.stack([p // (Y * Z), (p // Z) % Y, p % Z], 1)
    cand = []
    for d1 in (0, 1):
        for d2 in (0, 1):
            # an edge lies in the (up to) four cells shifted by 0 / -1 along the two axes it does not run along
            c = ijk.copy()
            for axis, (u, w) in enumerate(((1, 2), (0, 2), (0, 1))):
                m = ax == axis
                c[m, u] -= d1
                c[m, w] -= d2
            ok = (c >= 0).all(1) & (c[:, 0] < X - 1) & (c[:, 1] < Y - 1) & (c[:, 2] < Z - 1)
            cand.append(np.where(ok, (c[:, 0] * (Y - 1) + c[:, 1]) * (Z - 1) + c[:, 2], -1 - np.arange(len(c))))
    cand = np.stack(cand, 1)                     # [V, 4]
    if tri.size == 0:
        return
    c0, c1, c2 = cand[tri[:, 0]], cand[tri[:, 1]], cand[tri[:, 2]]
    common = ((c0[:, :, None, None] == c1[:, None, :, None]) & (c0[:, :, None, None] == c2[:, None, None, :])).any((1, 2, 3))
    assert common.all(), np.argwhere(~common)[:5]


def _grid(n):
    g = torch.arange(n, device="cuda", dtype=torch.float32)
    return torch.meshgrid(g, g, g, indexing="ij")


def _sphere(n, c, r):
    x, y, z = _grid(n)
    return r - torch.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)


def _topology(v, t, vol, iso):
    """Closed, consistently oriented 2-manifold: (Euler characteristic, enclosed volume)."""
    V, T = v.cpu().numpy().astype(np.float64), t.cpu().numpy()
    assert len(T) > 0
    keys, _ = crossing_edges(vol.cpu().numpy(), iso)
    assert len(keys) == len(V)
    _check_cells(T, keys, tuple(vol.shape))
    d = np.concatenate([T[:, [0, 1]], T[:, [1, 2]], T[:, [2, 0]]])
    code = d[:, 0] * len(V) + d[:, 1]
    assert len(np.unique(code)) == len(code), "a directed edge is used twice"
    rev = d[:, 1] * len(V) + d[:, 0]
    assert np.isin(rev, code).all(), "an edge without its opposite"
    assert len(np.unique(T)) == len(V), "unreferenced vertices"
    chi = len(V) - len(code) // 2 + len(T)
    vol_enc = np.einsum("ij,ij->i", V[T[:, 0]], np.cross(V[T[:, 1]], V[T[:, 2]])).sum() / 6.0
    return chi, vol_enc


def test_topology_of_analytic_surfaces():
    import nerf_projects_amd as N
    n = 64
    vol = _sphere(n, (31.3, 32.6, 30.8), 20.0)
    chi, enc = _topology(*N.marching_cubes_volume(vol, 0.0), vol, 0.0)
    assert chi == 2
    want = 4.0 / 3.0 * np.pi * 20.0 ** 3
    assert enc > 0 and abs(enc - want) <= 0.01 * want, (enc, want)
    x, y, z = _grid(n)
    torus = 5.0 - torch.sqrt((torch.sqrt((x - 31.6) ** 2 + (y - 32.2) ** 2) - 16.0) ** 2 + (z - 31.1) ** 2)
    chi, enc = _topology(*N.marching_cubes_volume(torus, 0.0), torus, 0.0)
    assert chi == 0 and enc > 0
    two = torch.maximum(_sphere(n, (18.2, 20.5, 31.0), 10.0), _sphere(n, (44.7, 41.3, 30.2), 11.0))
    chi, enc = _topology(*N.marching_cubes_volume(two, 0.0), two, 0.0)
    assert chi == 4 and enc > 0
    g = torch.Generator(device="cpu").manual_seed(5)
    smooth = torch.zeros_like(x)
    for _ in range(6):
        f = (torch.rand(3, generator=g) * 0.5 + 0.05).tolist()
        ph = (torch.rand(3, generator=g) * 6.28).tolist()
        smooth += torch.sin(x * f[0] + ph[0]) * torch.cos(y * f[1] + ph[1]) * torch.sin(z * f[2] + ph[2])
    r2 = ((x - 31.5) ** 2 + (y - 31.5) ** 2 + (z - 31.5) ** 2) / 28.0 ** 2
    field = (smooth + 1.0) * torch.clamp(1.0 - r2, min=0.0) - 0.5
    _, enc = _topology(*N.marching_cubes_volume(field, 0.0), field, 0.0)
    assert enc > 0


def _raw_mc(vol, iso, v_cap, t_cap, verts=None, tris=None):
    from nerf_projects_amd import _lib, get_context
    ctx = get_context()
    nv, nt = C.c_int64(-1), C.c_int64(-1)
    a = _lib.McArgs()
    a.volume = vol.data_ptr()
    a.reso[:] = list(vol.shape)
    a.iso = iso
    a.vertices = 0 if verts is None else verts.data_ptr()
    a.vertex_capacity = v_cap
    a.triangles = 0 if tris is None else tris.data_ptr()
    a.triangle_capacity = t_cap
    a.n_vertices, a.n_triangles = C.pointer(nv), C.pointer(nt)
    a.stream = ctx.stream().value
    rc = ctx.lib.nerf_marching_cubes(ctx.handle, C.byref(a))
    return rc, nv.value, nt.value


def test_determinism_sizes_and_refusals(N):
    vol = _sphere(48, (23.4, 24.1, 22.9), 15.0)
    v1, t1 = N.marching_cubes_volume(vol, 0.0)
    v2, t2 = N.marching_cubes_volume(vol, 0.0)
    assert torch.equal(v1, v2) and torch.equal(t1, t2)
    # count only: exact counts
    rc, nv, nt = _raw_mc(vol, 0.0, 0, 0)
    assert rc == 0 and (nv, nt) == (v1.shape[0], t1.shape[0])
    # too small: nothing written, an error, the counts reported
    verts = torch.full((nv, 3), -7.0, device="cuda")
    tris = torch.full((nt, 3), -7, device="cuda", dtype=torch.int64)
    for vc, tc in ((nv - 1, nt), (nv, nt - 1)):
        rc, gv, gt = _raw_mc(vol, 0.0, vc, tc, verts, tris)
        torch.cuda.synchronize()
        assert rc < 0 and (gv, gt) == (nv, nt)
        assert (verts == -7.0).all() and (tris == -7).all()
    rc, _, _ = _raw_mc(vol, 0.0, nv, nt, verts, tris)
    assert rc == 0 and torch.equal(verts, v1) and torch.equal(tris, t1)
    # no crossing: an empty mesh
    v, t = N.marching_cubes_volume(torch.full((9, 8, 7), -1.0, device="cuda"), 0.0)
    assert v.shape == (0, 3) and t.shape == (0, 3)
    # refusals
    net = make_net(N, synthetic.synthetic_pair(0)[1])
    for reso in (1, 1025, (4, 1, 4), (4, 4, 1025)):
        with pytest.raises(RuntimeError, match="reso"):
            N.density_grid(net, -1.0, 1.0, reso)
    for c1, c2 in ((1.0, 1.0), (1.0, -1.0), ((-1, -1, 0.5), (1, 1, 0.5))):
        with pytest.raises(RuntimeError, match="c2"):
            N.density_grid(net, c1, c2, 8)
    for shape in ((1, 5, 5), (5, 5, 1), (1025, 2, 2)):
        with pytest.raises(RuntimeError, match="reso"):
            N.marching_cubes_volume(torch.zeros(shape, device="cuda"), 0.0)


def test_lattice_beyond_int32_counts():
    """3 * X * Y * Z > 2^31 (900^3): the count-only call is exact (int64 offsets)."""
    n = 900
    g = torch.Generator(device="cuda").manual_seed(11)
    vol = torch.rand((n, n, n), device="cuda", generator=g)
    rc, nv, nt = _raw_mc(vol, 0.5, 0, 0)
    assert rc == 0
    inside = vol >= 0.5
    del vol
    want = sum(int((inside.narrow(a, 1, n - 1) != inside.narrow(a, 0, n - 1)).sum()) for a in range(3))
    assert 3 * n ** 3 > 2 ** 31 and nv == want and nt > nv // 2
    del inside
    torch.cuda.empty_cache()


def test_end_to_end_and_save_obj(N, tmp_path):
    """gen_mesh.marching_cubes == density_grid -> marching_cubes_volume -> the reference's rescaling (done here in numpy);
    save_obj round-trips through the OBJ text."""
    net = make_net(N, synthetic.synthetic_pair(0)[1])
    c1, c2, reso = (-1.2, -1.1, -1.3), (1.25, 1.05, 1.2), (40, 36, 44)
    sigma = N.density_grid(net, c1, c2, reso)
    iso = float(np.percentile(sigma.cpu().numpy()[sigma.cpu().numpy() > 0], 50))
    v, t = N.marching_cubes(net, c1, c2, reso, iso)
    gv, gt = N.marching_cubes_volume(sigma, iso)
    want = gv.cpu().numpy().astype(np.float64)
    want *= (np.array(c2) - np.array(c1)) / np.array(reso)
    want = want + np.array(c1)
    assert v.dtype == np.float64 and t.dtype == np.int64 and len(t) > 0
    assert np.array_equal(v, want) and np.array_equal(t, gt.cpu().numpy())
    path = tmp_path / "mesh.obj"
    N.save_obj(v, t, str(path))
    rows = path.read_text().splitlines()
    vs = np.array([[float(x) for x in r.split()[1:]] for r in rows if r.startswith("v ")])
    fs = np.array([[int(x) for x in r.split()[1:]] for r in rows if r.startswith("f ")])
    assert np.abs(vs - v).max() <= 5e-5 + 1e-12 and np.array_equal(fs - 1, t)
