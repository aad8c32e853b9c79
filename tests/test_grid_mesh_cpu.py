"""Surface meshes of a sparse voxel grid, the parts that need no GPU: the ABI of the two new entry points, the writers, the
argument checks that come before any device work, the generated code of the attribute kernel, and the oracle itself
(tests/grid_mesh_oracle.py): its fp32 restatement of the kernel held to the a-priori bounds the GPU tests use."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import grid_mesh_oracle as MO
from grid_testlib import assert_structs_match_c_header, compile_kernels_to_asm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def N():
    import nerf_projects_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def lib():
    from nerf_projects_amd import _lib
    if not os.path.exists(_lib.library_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def test_structs_and_constants_match_the_header(lib, tmp_path):
    from nerf_projects_amd import _lib
    names = ("NERF_GRID_MESH_COLOR_NONE", "NERF_GRID_MESH_COLOR_DC", "NERF_GRID_MESH_COLOR_SH", "NERF_GRID_MESH_COLOR_VIEW")
    seen = assert_structs_match_c_header(
        tmp_path, {"nerf_grid_mc_args": "GridMcArgs", "nerf_grid_mesh_attributes_args": "GridMeshAttributesArgs"},
        [f'printf("const {n} %d\\n", {n});' for n in names])
    assert seen == {"const": {n: getattr(_lib, n) for n in names}}
    for s in ("nerf_grid_marching_cubes", "nerf_grid_mesh_attributes"):
        assert hasattr(lib, s) and s in _lib.EXPORTS


def test_null_grid_is_refused_without_a_device(lib):
    from nerf_projects_amd import _lib
    n_v, n_t = C.c_int64(-1), C.c_int64(-1)
    a = _lib.GridMcArgs()
    a.iso, a.n_vertices, a.n_triangles = 1.0, C.pointer(n_v), C.pointer(n_t)
    assert lib.nerf_grid_marching_cubes(None, C.byref(a)) < 0 and b"NULL grid" in lib.nerf_last_error()
    assert lib.nerf_grid_mesh_attributes(None, C.byref(_lib.GridMeshAttributesArgs())) < 0
    assert b"NULL grid" in lib.nerf_last_error()
    assert (n_v.value, n_t.value) == (-1, -1)


def test_package_surface(N):
    assert N.grid_mesh.extract_mesh is N.extract_mesh and N.grid_mesh.mesh_attributes is N.mesh_attributes
    assert N.grid_mesh.GridMesh is N.GridMesh
    import inspect
    sig = inspect.signature(N.extract_mesh)
    assert list(sig.parameters) == ["grid", "isovalue", "mask", "normals", "colors", "world", "render_offset"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [None, True, "sh", True, 1.5]
    assert all(p.kind is p.KEYWORD_ONLY for p in list(sig.parameters.values())[2:])
    sig = inspect.signature(N.mesh_attributes)
    assert list(sig.parameters) == ["grid", "points_index", "mask", "colors", "view"]
    # the documented composition with the floater tools, and what a mask at another threshold does
    doc = N.grid_mesh.__doc__
    assert "label_components(grid, threshold=iso)" in doc and "labels == (vol.argmax() + 1)" in doc and "cut faces" in doc


# ---- argument checks that come before the device ------------------------------------------------------------------------------
@pytest.mark.parametrize("iso", [0.0, -1.0, float("nan"), float("inf"), 1e-60])
def test_isovalue_must_be_positive_and_finite(N, iso):
    with pytest.raises(ValueError, match="isovalue"):
        N.grid_mesh._check_iso(iso)


def test_isovalue_is_rounded_to_fp32(N):
    assert N.grid_mesh._check_iso(0.1) == float(np.float32(0.1))


@pytest.mark.parametrize("colors", ["rgb", "SH", 3, (1.0, 0.0), (0.0, 0.0, 0.0), (float("nan"), 0.0, 1.0), ("a", "b", "c")])
def test_bad_colors_are_refused(N, colors):
    with pytest.raises(ValueError, match="colors"):
        N.grid_mesh._check_colors(colors, render=True)


def test_colors_modes(N):
    from nerf_projects_amd import _lib
    check = N.grid_mesh._check_colors
    assert check(None) == (_lib.NERF_GRID_MESH_COLOR_NONE, None)
    assert check("dc") == (_lib.NERF_GRID_MESH_COLOR_DC, None) and check("sh") == (_lib.NERF_GRID_MESH_COLOR_SH, None)
    assert check("render", render=True) == ("render", None)
    with pytest.raises(ValueError, match="colors"):
        check("render")
    mode, d = check((1.0, 2.0, -2.0))
    assert mode == _lib.NERF_GRID_MESH_COLOR_VIEW and d.dtype == np.float32
    assert np.array_equal(d, (np.array([1.0, 2.0, -2.0]) / 3.0).astype(np.float32))      # normalised in fp64, then rounded
    mode2, d2 = check("sh", view=[1.0, 2.0, -2.0])
    assert mode2 == mode and np.array_equal(d2, d)
    with pytest.raises(ValueError, match="view"):
        check("dc", view=(0.0, 0.0, 1.0))


def test_not_a_grid_is_a_type_error(N):
    with pytest.raises(TypeError, match="SparseGrid"):
        N.extract_mesh(np.zeros((4, 4, 4), np.float32), 1.0)
    with pytest.raises(TypeError, match="SparseGrid"):
        N.mesh_attributes(None, torch.zeros(1, 3))


# ---- writers ---------------------------------------------------------------------------------------------------------------
def small_mesh(N, normals, colors, seed=0):
    rng = np.random.default_rng(seed)
    v = torch.from_numpy(rng.normal(0.0, 3.0, (7, 3)).astype(np.float32))
    t = torch.from_numpy(rng.integers(0, 7, (5, 3)).astype(np.int64))
    n = torch.from_numpy(rng.normal(0.0, 1.0, (7, 3)).astype(np.float32)) if normals else None
    c = torch.from_numpy(rng.uniform(-0.2, 1.2, (7, 3)).astype(np.float32)) if colors else None
    return N.GridMesh(v, t, n, c)


@pytest.mark.parametrize("colors", [False, True])
def test_save_obj_writes_what_the_existing_writer_writes(N, tmp_path, colors):
    m = small_mesh(N, True, colors)
    a, b = tmp_path / "a.obj", tmp_path / "b.obj"
    m.save_obj(str(a))
    N.save_obj(m.vertices, m.triangles, str(b), m.colors)
    assert a.read_text() == b.read_text() and a.read_text().count("\n") == 12
    assert len(a.read_text().splitlines()[0].split()) == (7 if colors else 4)


@pytest.mark.parametrize("normals,colors", [(False, False), (True, False), (False, True), (True, True)])
def test_save_ply_round_trips(N, tmp_path, normals, colors):
    m = small_mesh(N, normals, colors, seed=1)
    path = tmp_path / "m.ply"
    m.save_ply(str(path))
    head = path.read_bytes().split(b"end_header\n")[0].decode("ascii").splitlines()
    want = ["property float x", "property float y", "property float z"]
    want += ["property float nx", "property float ny", "property float nz"] if normals else []
    want += ["property uchar red", "property uchar green", "property uchar blue"] if colors else []
    assert head[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 7"]
    assert head[3:] == want + ["element face 5", "property list uchar int vertex_indices"]
    got = MO.read_ply(str(path))
    vert = got["vertex"]
    assert np.array_equal(np.stack([vert["x"], vert["y"], vert["z"]], -1).tobytes(), m.vertices.numpy().tobytes())
    assert np.array_equal(got["face"], m.triangles.numpy()) and got["face"].dtype == np.dtype("<i4")
    if normals:
        assert np.stack([vert["nx"], vert["ny"], vert["nz"]], -1).tobytes() == m.normals.numpy().tobytes()
    if colors:
        assert np.array_equal(np.stack([vert["red"], vert["green"], vert["blue"]], -1), N.to8b(m.colors.numpy()))
    assert set(vert.dtype.names) == {w.split()[-1] for w in want}


def test_save_ply_of_an_empty_mesh(N, tmp_path):
    m = N.GridMesh(torch.zeros((0, 3)), torch.zeros((0, 3), dtype=torch.int64), torch.zeros((0, 3)), torch.zeros((0, 3)))
    m.save_ply(str(tmp_path / "e.ply"))
    got = MO.read_ply(str(tmp_path / "e.ply"))
    assert got["vertex"].shape == (0,) and got["face"].shape == (0, 3)
    m.save_obj(str(tmp_path / "e.obj"))
    assert (tmp_path / "e.obj").read_text() == ""


# ---- the oracle: its fp32 restatement of the kernel against its fp64 self, under the bounds of the GPU tests -------------------
FIXTURES = [((17, 9, 33), 5), ((40, 40, 40), 6)]


@pytest.mark.parametrize("reso,seed", FIXTURES)
def test_oracle_normal_bound_holds_for_the_fp32_restatement(reso, seed):
    g = MO.blob_fixture(reso, seed, radius=(1.0, 0.5, 2.0), center=(0.1, -0.2, 0.3))
    V = MO.node_values(g["links"], g["density_data"])
    pts = MO.crossing_vertices(V, 10.0)
    assert pts.shape[0] > 500
    n64, bound, _ = MO.normals64(V, pts, g["radius"])
    n32 = MO.normals32(V, pts, g["radius"])
    ok = bound <= 1e-3
    err = np.max(np.abs(n32.astype(np.float64) - n64), axis=1)
    print(f"{reso}: {pts.shape[0]} vertices, {int((~ok).sum())} left out, worst error / bound {np.max(err[ok] / bound[ok]):.3f}")
    assert (~ok).sum() <= 0.01 * pts.shape[0]
    assert np.all(err[ok] <= bound[ok])
    assert np.allclose(np.linalg.norm(n64[ok], axis=1), 1.0, atol=1e-12)


def test_oracle_gradient_rule():
    V = np.arange(24, dtype=np.float32).reshape(2, 3, 4) ** 2
    G = MO.node_gradient(V)
    assert G[0, 1, 1, 0] == V[1, 1, 1] - V[0, 1, 1] and G[1, 1, 1, 0] == V[1, 1, 1] - V[0, 1, 1]      # border: one-sided, h = 1
    assert G[0, 1, 1, 1] == 0.5 * (V[0, 2, 1] - V[0, 0, 1]) and G[0, 0, 1, 1] == V[0, 1, 1] - V[0, 0, 1]
    assert G[1, 2, 2, 2] == 0.5 * (V[1, 2, 3] - V[1, 2, 1]) and G[1, 2, 3, 2] == V[1, 2, 3] - V[1, 2, 2]
    # on a lattice edge the interpolation is the linear interpolation of the two end nodes
    p = np.array([[0.0, 1.0, 1.25]], np.float32)
    l, w = MO.point_cell(p, V.shape)
    assert np.allclose(MO.trilerp(G, l, w)[0], 0.75 * G[0, 1, 1] + 0.25 * G[0, 1, 2], rtol=1e-15)
    # the last node of an axis belongs to the last cell with weight 1
    l, w = MO.point_cell(np.array([[1.0, 2.0, 3.0], [-3.0, 9.0, np.nan]], np.float32), V.shape)
    assert l.tolist() == [[0, 1, 2], [0, 1, 0]] and w.tolist() == [[1.0, 1.0, 1.0], [0.0, 1.0, 0.0]]


def test_oracle_crossing_vertices_special_values():
    iso = np.float32(2.0)
    V = np.zeros((2, 2, 6), np.float32)
    V[0, 0, :] = [2.0, 0.0, np.nan, 5.0, np.inf, -3.0]
    v = MO.crossing_vertices(V, iso)
    # the z edges of the line (0, 0, .): exactly iso is inside and t = 0; 0 - NaN is outside - outside, no vertex; NaN - 5 and
    # inf - (-3) give t = 0.5; 5 - inf is inside - inside
    z_edges = v[(v[:, 0] == 0) & (v[:, 1] == 0)]
    assert z_edges[:, 2].tolist() == [0.0, 0.0, 0.0, 2.5, 4.5]      # (node 0's x and y edges have t = 0 too)
    # the x and y edges from the four inside nodes to their outside neighbours: t = 0 at 2.0, 0.5 at inf, (2 - 5) / (0 - 5) at 5
    assert v.shape[0] == 3 + 2 * 3 and [0.5, 0.0, 4.0] in v.tolist() and [0.0, 0.0, 0.0] in v.tolist()
    assert [np.float32(0.6), 0.0, 3.0] in v.tolist()


@pytest.mark.parametrize("basis_dim", [1, 4, 9])
@pytest.mark.parametrize("mode", ["dc", "sh", "view"])
def test_oracle_colour_bound_holds_for_the_fp32_restatement(basis_dim, mode):
    rng = np.random.default_rng(basis_dim)
    n = 4000
    S = (rng.normal(0.0, 0.7, (n, 3 * basis_dim)) * rng.choice([0.2, 1.0, 6.0], (n, 1))).astype(np.float32)
    nr = rng.normal(0.0, 1.0, (n, 3))
    nr = (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(np.float32)
    nr[::17] = 0.0
    view = (np.array([1.0, 2.0, -2.0]) / 3.0).astype(np.float32)
    want, bound = MO.colors64(S, basis_dim, mode, nr, view)
    got = MO.colors32(S, basis_dim, mode, nr, view)
    assert (want == 0.0).any() and (want == 1.0).any() and ((want > 0.0) & (want < 1.0)).any()      # both clamps are hit
    err = np.abs(got.astype(np.float64) - want)
    print(f"B = {basis_dim}, {mode}: worst error / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    if mode == "sh":      # a zero normal falls back to the constant term
        dc, _ = MO.colors64(S, basis_dim, "dc")
        assert np.array_equal(want[::17], dc[::17])
    if basis_dim == 1:
        assert np.array_equal(want, MO.colors64(S, 1, "dc")[0])


def test_oracle_sh_basis_is_the_packages(N):
    d = np.random.default_rng(0).normal(size=(50, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    for B in (1, 4, 9):
        assert np.allclose(MO.sh_basis(B, d), N.grid.eval_sh_bases(B, d), rtol=1e-15, atol=0)
    assert np.max(np.abs(MO.sh_basis(9, d))) < 0.64


def test_oracle_topology_helpers():
    tet = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]])
    _, counts = MO.edge_counts(tet)
    assert np.all(counts == 2) and MO.mesh_components(4, tet) == 1
    two = np.concatenate([tet, tet + 4])
    assert MO.mesh_components(9, two) == 2
    _, counts = MO.edge_counts(tet[:3])
    assert sorted(counts.tolist()) == [1, 1, 1, 2, 2, 2]


# ---- generated code --------------------------------------------------------------------------------------------------------
def test_attribute_kernels_use_no_scratch_and_no_lds(tmp_path):
    text, asm, _ = compile_kernels_to_asm(tmp_path, "grid_mesh_kernels.hip")
    code = re.sub(r"//[^\n]*", "", text)
    assert not re.search(r"\basm\b|__asm|\batomic", code)
    kernels = re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M)
    assert len(kernels) == 3 and all("grid_mesh_attributes_kernel" in k for k in kernels), kernels      # fp32, half, palette
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)
    assert len(sizes) == 3 and all(int(s) == 0 for s in sizes), sizes
    assert not re.search(r"\bscratch_(load|store)", asm)
    lds = re.findall(r"\.group_segment_fixed_size:\s*(\d+)", asm)
    assert len(lds) == 3 and all(int(s) == 0 for s in lds), lds
    print("vgprs per kernel:", dict(zip(kernels, re.findall(r"\.vgpr_count:\s*(\d+)", asm))))


def test_the_extraction_shares_the_dense_kernels():
    """nerf_grid_marching_cubes is the dense call's kernels with another source of node values, not a second copy."""
    text = open(os.path.join(ROOT, "nerf-projects_amd", "csrc", "mesh_kernels.hip")).read()
    code = re.sub(r"//[^\n]*", "", text)
    for k in ("mc_edge_count_kernel", "mc_cell_count_kernel", "mc_vertex_kernel", "mc_triangle_kernel"):
        assert len(re.findall(r"void %s\(" % k, code)) == 1 and re.search(r"template <class Vol>\s*__global__[^\n]*%s" % k, code), k
    assert "struct McVolume" in code and "struct McGridVolume" in code
    assert not re.search(r"\batomic", code)
