"""PlenOctree without a GPU (include/nerf_mi355x.h, "PlenOctree"): the oracle's SH basis against the reference's own, the
container's file round trip and its checks of a foreign tree, the oracle against closed forms, the agreement of the fp32 and
the all-fp64 traversal on the cases the GPU tests use, the oracle's build, the C entries' refusals that need no device, the
struct mirrors and the generated code of the kernels."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import octree_oracle as O  # noqa: E402
from grid_testlib import assert_structs_match_c_header, compile_kernels_to_asm  # noqa: E402

STRUCTS = {"nerf_octree_desc": "OctreeDesc", "nerf_octree_render_options": "OctreeRenderOptions",
           "nerf_octree_render_args": "OctreeRenderArgs", "nerf_octree_build_args": "OctreeBuildArgs"}
SYMBOLS = ("nerf_octree_create", "nerf_octree_destroy", "nerf_octree_render_rays", "nerf_octree_render_image",
           "nerf_octree_build_workspace", "nerf_octree_build_from_grid", "nerf_octree_accelerate", "nerf_octree_table_levels")
FILE_KEYS = {"data_dim", "child", "parent_depth", "n_internal", "n_free", "invradius3", "offset", "depth_limit",
             "geom_resize_fact", "data", "data_format"}


@pytest.fixture(scope="module")
def N():
    import nerf_projects_amd
    return nerf_projects_amd


@pytest.fixture(scope="module")
def lib():
    from nerf_projects_amd import _lib
    return _lib.load()


def err(lib):
    return lib.nerf_last_error().decode()


# ---- 1. the SH basis against the reference's eval_sh ------------------------------------------------------------------------
def test_oracle_basis_meets_the_reference(golden):
    z = golden("octree")
    for deg in range(5):
        B = (deg + 1) ** 2
        got = (O.sh_basis(B, z["dirs"], np.float64)[:, None, :] * z[f"sh_{deg}"]).sum(-1)
        assert np.abs(got - z[f"out_{deg}"]).max() <= 1e-12, deg
        # and the fp32 basis is that basis, rounded
        assert np.abs(O.sh_basis(B, z["dirs"].astype(np.float32), np.float32) - O.sh_basis(B, z["dirs"].astype(np.float32))).max() < 4e-6


# ---- 2. the file ------------------------------------------------------------------------------------------------------------
def small_tree(N, B=4, seed=0):
    links, density, sh = O.fixture_grid(seed, 8, B, "octants")
    t = O.build_from_grid(links, density, sh, radius=[1.0, 1.5, 0.5], center=[0.1, 0.0, -0.2])
    tree = N.N3Tree(t["child"], t["data"], t["parent_depth"], t["invradius"], t["offset"], f"SH{B}", "relu_half", device="cpu")
    return t, tree


def test_save_load_round_trip_and_names(N, tmp_path):
    t, tree = small_tree(N)
    assert tree.max_depth == t["max_depth"] == 2 and tree.data_dim == 13 and tree.n_internal == t["child"].shape[0]
    assert tree.n_leaves == int((t["child"] == 0).sum())
    path = str(tmp_path / "tree.npz")
    tree.save(path)
    z = np.load(path)
    assert set(z.files) == FILE_KEYS | {"rgb_activation"}
    assert z["data"].dtype == np.float16 and z["child"].dtype == np.int32 and z["parent_depth"].dtype == np.int32
    assert int(z["data_dim"]) == 13 and int(z["n_internal"]) == tree.n_internal and int(z["n_free"]) == 0
    back = N.N3Tree.load(path, device="cpu")
    assert torch.equal(back.child, tree.child) and torch.equal(back.parent_depth, tree.parent_depth)
    assert np.array_equal(back.data.numpy(), t["data"].astype(np.float16).astype(np.float32))      # fp16 survives
    assert back.data.dtype == torch.float32 and back.data_format == "SH4" and back.rgb_activation == "relu_half"
    assert torch.equal(back.invradius, tree.invradius) and torch.equal(back.offset, tree.offset) and back.max_depth == 2
    # a file of svox itself: no rgb_activation key, a scalar invradius
    d = dict(z)
    del d["rgb_activation"], d["invradius3"]
    d["invradius"] = np.float32(0.25)
    np.savez(str(tmp_path / "svox.npz"), **d)
    sv = N.N3Tree.load(str(tmp_path / "svox.npz"), device="cpu")
    assert sv.rgb_activation == "sigmoid" and sv.invradius.tolist() == [0.25] * 3
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sv.volume_render(N.Rays(torch.zeros(1, 3), torch.ones(1, 3)))


def test_compressed_file_loads_to_the_rule_of_compressed_evaluation(N, tmp_path):
    """A file in compression.py's form, made here from a tiny palette, with and without retained coefficients."""
    t, tree = small_tree(N)
    rng = np.random.default_rng(3)
    n, B, K = t["child"].shape[0], 4, 8
    for retain in (0, 1):
        Q = B - retain
        colors = rng.standard_normal((Q, K, 3)).astype(np.float16)
        qmap = rng.integers(0, K, (Q, n, 2, 2, 2)).astype(np.uint16)
        qmap[0, 0, 0, 0, 0] = K + 3      # past the palette: stays zero
        sigma = np.abs(rng.standard_normal((n, 2, 2, 2))).astype(np.float16)
        retained = rng.standard_normal((retain, n, 2, 2, 2, 3)).astype(np.float16)
        z = {"child": t["child"], "invradius3": t["invradius"], "offset": t["offset"], "data_dim": np.int64(13),
             "data_format": "SH4", "quant_colors": colors, "quant_map": qmap, "sigma": sigma}
        if retain:
            z["data_retained"] = retained
        path = str(tmp_path / f"compressed{retain}.npz")
        np.savez(path, **z)
        want = np.zeros((n, 2, 2, 2, 13), np.float32)      # compressed_evaluation.py:128-158, retained coefficients first
        for b in range(B):
            if b < retain:
                trip = retained[b].astype(np.float32)
            else:
                ids = qmap[b - retain]
                valid = ids < K
                trip = np.zeros((n, 2, 2, 2, 3), np.float32)
                trip[valid] = colors[b - retain][ids[valid]]
            for c in range(3):
                want[..., c * B + b] = trip[..., c]
        want[..., -1] = sigma
        got = N.N3Tree.load(path, device="cpu")
        assert np.array_equal(got.data.numpy(), want.astype(np.float16).astype(np.float32)) and got.basis_dim == 4
        assert got.max_depth == 2 and torch.equal(got.parent_depth, torch.zeros(n, 2, dtype=torch.int32))


def test_a_foreign_tree_is_checked(N, tmp_path):
    t, tree = small_tree(N)
    mk = lambda child, data=None: N.N3Tree(child, t["data"] if data is None else data, None, 0.5, 0.5, "SH4", device="cpu")   # noqa: E731
    past = t["child"].copy()
    past[-1, 1, 1, 1] = 1      # points at node n
    with pytest.raises(ValueError, match="past"):
        mk(past)
    neg = t["child"].copy()
    neg[3, 0, 1, 0] = -2
    with pytest.raises(ValueError, match="negative"):
        mk(neg)
    deep = np.zeros((26, 2, 2, 2), np.int32)      # a chain: node i hangs in cell 0 of node i - 1, depths 0 .. 25
    deep[:-1, 0, 0, 0] = 1
    with pytest.raises(ValueError, match="deeper than 24"):
        mk(deep, np.zeros((26, 2, 2, 2, 13), np.float32))
    ok = mk(deep[:25].copy() * (np.arange(25) < 24)[:, None, None, None], np.zeros((25, 2, 2, 2, 13), np.float32))
    assert ok.max_depth == 24
    np.savez(str(tmp_path / "bad.npz"), child=past, data=t["data"].astype(np.float16), invradius3=t["invradius"], offset=t["offset"],
             data_format="SH4")
    with pytest.raises(ValueError, match="past"):
        N.N3Tree.load(str(tmp_path / "bad.npz"), device="cpu")
    with pytest.raises(ValueError, match="data must be"):
        mk(t["child"], t["data"][..., :-1])
    for missing, word in (("invradius3", "invradius3 or invradius"), ("offset", "offset"), ("data", "data"), ("child", "child")):
        z = dict(child=t["child"], data=t["data"].astype(np.float16), invradius3=t["invradius"], offset=t["offset"])
        del z[missing]
        np.savez(str(tmp_path / "missing.npz"), **z)
        with pytest.raises(ValueError, match="no array named " + word):
            N.N3Tree.load(str(tmp_path / "missing.npz"), device="cpu")
    for fmt, word in (("RGBA", "RGBA"), ("SG9", "Gaussians"), ("ASG4", "Gaussians")):
        with pytest.raises(NotImplementedError, match=word):
            N.N3Tree(t["child"], t["data"], None, 0.5, 0.5, fmt, device="cpu")
    with pytest.raises(NotImplementedError, match="N = 4"):
        N.N3Tree(t["child"], t["data"], None, 0.5, 0.5, "SH4", N=4, device="cpu")
    with pytest.raises(NotImplementedError, match="extra_data"):
        N.N3Tree(t["child"], t["data"], None, 0.5, 0.5, "SH4", extra_data=np.zeros(3), device="cpu")
    with pytest.raises(NotImplementedError, match="NDC"):
        N.N3Tree(t["child"], t["data"], None, 0.5, 0.5, "SH4", ndc=(1.0, 1.0), device="cpu")
    for name in ("refine", "shrink_to_fit"):
        with pytest.raises(NotImplementedError, match=name):
            getattr(tree, name)()


# ---- 3. the oracle against closed forms --------------------------------------------------------------------------------------
def root_only(sigma, coef, act="sigmoid"):
    data = np.zeros((1, 2, 2, 2, 4), np.float32)
    data[..., :3] = coef
    data[..., 3] = sigma
    return O.make_tree(np.zeros((1, 2, 2, 2), np.int32), data, 0.5, 0.5, act)


def test_oracle_against_closed_forms():
    sigma, step, bg = 3.0, 1e-3, 0.25
    coef = np.array([0.8, -0.5, 2.0], np.float32).astype(np.float64)      # as the fp32 rows hold them
    col = 1.0 / (1.0 + np.exp(-O.C0 * coef))
    tree = root_only(sigma, coef)
    s2, s3 = np.sqrt(2.0), np.sqrt(3.0)
    # world = 2 unit - 1; delta_scale = 2 for unit directions. The first leaf of a ray is entered exactly and gets its length
    # + step; every later one is entered step past its face and gets (length - step) + step.
    rays = [([-2.0, 0.3, -0.4], [1.0, 0.0, 0.0], [0.5 + step, 0.5]),                                   # along an axis: two leaves
            ([-2.0, -2.0, -2.0], [1 / s3] * 3, [0.5 * s3 + step, 0.5 * s3]),                           # the diagonal: two leaves
            ([-1.0 - 1.0, -0.5 - 1.0, -0.5], [1 / s2, 1 / s2, 0.0], [0.25 * s2 + step, 0.25 * s2, 0.25 * s2])]      # three leaves
    o = np.array([r[0] for r in rays], np.float32)
    d = np.array([r[1] for r in rays], np.float32)
    for trav, rad, tol in ((np.float32, np.float32, 2e-6), (np.float32, np.float64, 2e-6), (np.float64, np.float64, 1e-7)):
        rgb, steps, _ = O.march(tree, o, d, step_size=step, background_brightness=bg, trav=trav, rad=rad)
        assert steps.tolist() == [2, 2, 3]
        for i, (_, _, lengths) in enumerate(rays):
            T = np.prod([np.exp(-sigma * 2.0 * ln) for ln in lengths])      # the written product of exponentials
            assert np.abs(rgb[i] - ((1.0 - T) * col + T * bg)).max() < tol, (i, trav, rad)
    # a miss gives the background, and a non-finite ray NaN; both visit nothing
    rgb, steps, _ = O.march(tree, np.array([[3.0, 0, 0], [np.inf, 0, 0], [0, 0, 3.0]], np.float32),
                            np.array([[0, 1.0, 0], [1.0, 0, 0], [0, 0, 0]], np.float32), background_brightness=bg)
    assert np.array_equal(rgb[0], [bg] * 3) and np.isnan(rgb[1:]).all() and steps.tolist() == [0, 0, 0]
    # stop_thresh renormalises: an opaque first leaf leaves T <= 1e-2, and rgb (1 - T) / (1 - T) is the leaf's colour alone
    rgb, steps, _ = O.march(root_only(50.0, coef), o[:1], d[:1], stop_thresh=1e-2, background_brightness=bg, rad=np.float64)
    assert steps.tolist() == [1] and np.abs(rgb[0] - col).max() < 1e-12
    # relu_half is the grid's colour model
    rgb, _, _ = O.march(root_only(50.0, coef, "relu_half"), o[:1], d[:1], stop_thresh=1e-2, rad=np.float64)
    assert np.abs(rgb[0] - np.maximum(O.C0 * coef + 0.5, 0.0)).max() < 1e-7
    # the no-advance rule: 1e7 away, t is near 5e6 where an ulp is 0.5: a leaf of 1 / 16 cannot advance it
    _, t16, _, _ = O.case("r16")
    rgb, steps, _ = O.march(t16, np.array([[-1e7, 0.3, -0.4]], np.float32), np.array([[1.0, 0, 0]], np.float32))
    assert steps.tolist() == [1] and np.isfinite(rgb).all()


# ---- 4. the cap that keeps the GPU tests honest ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(O.CASES))
def test_fp32_and_fp64_traversals_agree_on_the_cases(name):
    """On every case the GPU tests use: the fp32 traversal (the definition) and the all-fp64 march visit the same leaves on
    >= 99 % of the rays, and agree there within the GPU tests' bar max(3 d_ref, 1e-5), d_ref = the distance between fp32 and
    fp64 radiometry on the fp32 traversal. So the definition is no artefact of fp32 on these inputs, and the GPU tests
    exclude nothing."""
    _, tree, o, d = O.case(name)
    acts = ("relu_half", "sigmoid") if name in ("r16", "sh16", "sh25") else ("relu_half",)
    for act in acts:
        t = O.with_activation(tree, act)
        for step in (1e-3, 1e-5):
            rgb32, s32, l32 = O.march(t, o, d, step_size=step)
            rgb64, s64, _ = O.march(t, o, d, step_size=step, rad=np.float64)
            rgba, _, la = O.march(t, o, d, step_size=step, trav=np.float64, rad=np.float64)
            assert np.array_equal(s32, s64)
            same = O.same_leaves(l32, la)
            d_ref = np.nanmax(np.abs(rgb32 - rgb64))
            bar = max(3 * d_ref, 1e-5)
            got = np.nanmax(np.abs(rgb64 - rgba)[same])
            print(f"{name} {act} step {step}: same leaves {same.mean():.4f}, d_ref {d_ref:.2e}, fp32 vs fp64 traversal {got:.2e} / bar {bar:.2e}")
            assert same.mean() >= 0.99 and got <= bar
            assert np.isnan(rgb32[-1]).all() and s32[-1] == 0 and s32[-7] == 0 and s32[:-7].max() > 2


# ---- 5. the oracle's build ---------------------------------------------------------------------------------------------------
def descend(t, p):
    node, cell = 0, None
    for depth in range(MAXD := t["max_depth"] + 1):
        p = p * 2
        u = np.floor(p).astype(int)
        p = p - u
        cell = (node, *u)
        if t["child"][cell] == 0:
            return cell, depth + 1
        node += t["child"][cell]
    return cell, MAXD


def test_oracle_build_from_grid():
    links, density, sh = O.fixture_grid(11, 8, 4, "octants")
    t = O.build_from_grid(links, density, sh)
    R, n = 8, t["child"].shape[0]
    for i in range(R):
        for j in range(R):
            for k in range(R):
                cell, depth = descend(t, (np.array([i, j, k]) + 0.5) / R)
                row = t["data"][cell]
                if links[i, j, k] >= 0:      # every kept node's row is found at (i + 0.5) / R, at depth L
                    assert depth == 3 and np.array_equal(row[:-1], sh[links[i, j, k]]) and row[-1] == density[links[i, j, k], 0]
                else:
                    assert not row.any()
                    # a zero leaf at the shallowest possible level: its parent cell holds a kept node somewhere
                    s = R >> (depth - 1)
                    assert depth == 1 or (links[i // s * s:(i // s + 1) * s, j // s * s:(j // s + 1) * s, k // s * s:(k // s + 1) * s] >= 0).any()
    assert descend(t, np.array([0.1, 0.2, 0.3]))[1] == 1      # the empty octant is one leaf of the root
    # breadth first: depths never decrease, and within a depth the nodes follow the C order of their cells
    depths = t["parent_depth"][:, 1]
    assert depths[0] == 0 and (np.diff(depths) >= 0).all() and t["parent_depth"][0, 0] == 0
    flat = t["child"].reshape(n, 8)
    kids = [(x + flat[x][flat[x] > 0]).tolist() for x in range(n)]
    assert sorted(sum(kids, [])) == list(range(1, n))      # every node but the root hangs in exactly one cell
    coords = np.zeros((n, 3), np.int64)
    for x in range(n):      # parent_depth is consistent with child (parents come first, so coords[x] is known)
        for c, y in zip(np.nonzero(flat[x])[0], kids[x]):
            assert t["parent_depth"][y, 0] == x * 8 + c and t["parent_depth"][y, 1] == depths[x] + 1
            coords[y] = coords[x] * 2 + [c >> 2, (c >> 1) & 1, c & 1]
    for l in range(1, 3):      # within a depth: the C order of the nodes' cell coordinates
        c = coords[depths == l]
        key = (c[:, 0] * (1 << l) + c[:, 1]) * (1 << l) + c[:, 2]
        assert len(key) > 1 and (np.diff(key) > 0).all()
    assert not t["data"][t["child"] != 0].any()      # internal cells carry zeros
    links2, density2, sh2 = O.fixture_grid(1, 2, 1)
    t2 = O.build_from_grid(links2, density2, sh2)
    assert t2["child"].shape == (1, 2, 2, 2) and not t2["child"].any() and t2["max_depth"] == 0      # R = 2: the root alone
    assert np.array_equal(t2["data"][0][links2 >= 0][:, -1], density2[links2[links2 >= 0], 0])
    assert np.array_equal(t["invradius"], [0.5] * 3) and np.array_equal(t["offset"], [0.5] * 3) and t["rgb_activation"] == "relu_half"


# ---- the C entries, without a device ----------------------------------------------------------------------------------------
def test_octree_structs_match_a_c_compile_of_the_header(tmp_path):
    seen = assert_structs_match_c_header(tmp_path, STRUCTS, extra_prints=[
        'printf("act sigmoid %d\\n", NERF_OCTREE_RGB_SIGMOID);', 'printf("act relu_half %d\\n", NERF_OCTREE_RGB_RELU_HALF);',
        'printf("act max_depth %d\\n", NERF_OCTREE_MAX_DEPTH);'])
    from nerf_projects_amd import _lib
    assert seen["act"] == {"sigmoid": _lib.NERF_OCTREE_RGB_SIGMOID, "relu_half": _lib.NERF_OCTREE_RGB_RELU_HALF,
                           "max_depth": _lib.NERF_OCTREE_MAX_DEPTH}


def test_c_entries_refuse_without_a_device(lib):
    from nerf_projects_amd import _lib
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in _lib.EXPORTS, s
    fake, ptr = C.c_void_p(0x1000), 0x2000      # never dereferenced: these checks come before the first use of a handle
    out = C.c_void_p()

    def desc(**k):
        d = _lib.OctreeDesc()
        d.n_nodes, d.data_dim, d.max_depth, d.child, d.data = 5, 13, 2, ptr, ptr
        d.invradius[:], d.offset[:] = [0.5] * 3, [0.5] * 3
        for name, v in k.items():
            setattr(d, name, v)
        return d

    create = lib.nerf_octree_create
    assert create(None, C.byref(desc()), C.byref(out)) == -1 and "NULL argument" in err(lib)
    assert create(fake, None, C.byref(out)) == -1 and "nerf_octree_desc is NULL" in err(lib)
    d = desc()
    d.struct_size -= 8
    assert create(fake, C.byref(d), C.byref(out)) == -1 and "struct_size" in err(lib)
    for dim in (0, 3, 12, 14, 77, 5):
        assert create(fake, C.byref(desc(data_dim=dim)), C.byref(out)) == -1 and f"data_dim = {dim}" in err(lib)
    for k, word in ((dict(n_nodes=0), "n_nodes = 0"), (dict(max_depth=25), "max_depth = 25"), (dict(max_depth=-1), "max_depth"),
                    (dict(rgb_activation=2), "rgb_activation = 2")):
        assert create(fake, C.byref(desc(**k)), C.byref(out)) == -1 and word in err(lib)
    bad = desc()
    bad.invradius[1] = 0.0
    assert create(fake, C.byref(bad), C.byref(out)) == -1 and "invradius" in err(lib)
    assert out.value is None

    def opts(**k):
        o = _lib.OctreeRenderOptions()
        o.step_size, o.background_brightness = 1e-3, 1.0
        for name, v in k.items():
            setattr(o, name, v)
        return o

    a = _lib.OctreeRenderArgs()
    a.origins, a.dirs, a.n_rays, a.rgb = ptr, ptr, 4, ptr
    rays = lib.nerf_octree_render_rays
    assert rays(None, C.byref(opts()), C.byref(a)) == -1 and "NULL tree" in err(lib)
    assert rays(fake, C.byref(opts()), None) == -1 and "nerf_octree_render_args is NULL" in err(lib)
    assert rays(fake, None, C.byref(a)) == -1 and "nerf_octree_render_options is NULL" in err(lib)
    for step in (0.0, -1e-3, float("nan"), float("inf")):
        assert rays(fake, C.byref(opts(step_size=step)), C.byref(a)) == -1 and "step_size" in err(lib)
    assert rays(fake, C.byref(opts(sigma_thresh=float("nan"))), C.byref(a)) == -1 and "thresholds" in err(lib)
    a.n_rays = -1
    assert rays(fake, C.byref(opts()), C.byref(a)) == -1 and "n_rays = -1" in err(lib)
    a.n_rays, a.dirs = 4, None
    assert rays(fake, C.byref(opts()), C.byref(a)) == -1 and "origins and dirs" in err(lib)
    assert lib.nerf_octree_render_image(fake, None, C.byref(opts()), C.byref(a)) == -1 and "nerf_grid_camera is NULL" in err(lib)
    assert lib.nerf_octree_build_from_grid(None, C.byref(_lib.OctreeBuildArgs())) == -1 and "NULL grid" in err(lib)
    assert lib.nerf_octree_build_from_grid(fake, None) == -1 and "nerf_octree_build_args is NULL" in err(lib)
    assert lib.nerf_octree_accelerate(None, 6, None) == -1 and "NULL tree" in err(lib) and lib.nerf_octree_table_levels(None) == 0
    for levels in (-1, 9):
        assert lib.nerf_octree_accelerate(fake, levels, None) == -1 and f"levels = {levels}" in err(lib)
    for reso in (0, 1, 3, 12, 2048, -4):
        assert lib.nerf_octree_build_workspace(reso) == -1
    sizes = [lib.nerf_octree_build_workspace(1 << l) for l in range(1, 11)]
    assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] < 5 * 512 ** 3 * 8 // 7 + (1 << 20)      # 5 bytes per cell of levels 1 .. 9


def test_octree_kernels_generated_code(tmp_path):
    """The render kernels: no scratch (the SH basis is indexed at compile time), no LDS, no inline assembly; VGPRs per basis
    size, printed (profiles/octree.md quotes them)."""
    text, asm, build = compile_kernels_to_asm(tmp_path, "octree_kernels.hip")
    assert "octree_kernels.hip" in build.SOURCES and "octree_api.cpp" in build.SOURCES
    assert not re.search(r"\basm\b|__asm", text)
    for fn in ("camera_ray", "launch_grid_compact"):
        assert re.search(r"\b%s\b" % fn, text) and not re.search(r"\b(void|float|int|hipError_t)\s+%s\b" % fn, text), fn      # used, not copied
    kernels = re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M)
    render = [k for k in kernels if "octree_render" in k]
    assert len(render) == 20      # 5 basis sizes x rays / image x plain / table-started descent
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)
    assert len(sizes) == len(kernels) and all(int(s) == 0 for s in sizes), sizes
    assert not re.search(r"\bscratch_(load|store)", asm)
    vgprs = dict(zip(kernels, (int(v) for v in re.findall(r"\.vgpr_count:\s*(\d+)", asm))))
    print("vgprs per kernel:", vgprs)
    assert max(vgprs[k] for k in render) <= 128      # at least 4 waves per SIMD
