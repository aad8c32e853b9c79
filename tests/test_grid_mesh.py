"""Coloured surface meshes of a sparse voxel grid on the GPU (include/nerf_mi355x.h, "Sparse voxel grid: surface meshes").

Geometry: ``extract_mesh`` against the parent's dense path - the torch-densified volume through ``marching_cubes_volume``,
which tests/test_mesh.py pins - compared byte for byte. Normals and colours: against the fp64 oracle
(tests/grid_mesh_oracle.py) under its a-priori rounding bounds. Needs a real MI355X: run with ``pytest -m gpu``."""
import ctypes as C

import numpy as np
import pytest
import torch

import grid_mesh_oracle as MO
from test_grid import cpu, gpu, make_grid

pytestmark = pytest.mark.gpu

ISO = 10.0


@pytest.fixture(scope="module")
def N():
    import nerf_projects_amd as pkg
    return pkg


def densify(g, mask=None):
    """The volume a user of the parent commit builds with torch indexing."""
    links, density = gpu(g["links"]), gpu(g["density_data"])
    keep = links >= 0
    if mask is not None:
        keep = keep & (mask != 0)
    return torch.where(keep, density[links.clamp(min=0).long(), 0], torch.zeros((), device=links.device))


def same(a, b):
    return a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and cpu(a).tobytes() == cpu(b).tobytes()


def assert_geometry_is_the_dense_paths(N, grid, g, iso, mask=None):
    want_v, want_t = N.marching_cubes_volume(densify(g, mask), iso)
    m = N.extract_mesh(grid, iso, mask=mask, normals=False, colors=None, world=False)
    assert m.normals is None and m.colors is None
    assert m.vertices.dtype == torch.float32 and m.triangles.dtype == torch.int64 and m.vertices.is_cuda and m.triangles.is_cuda
    assert same(m.vertices, want_v), (tuple(m.vertices.shape), tuple(want_v.shape))
    assert same(m.triangles, want_t), (tuple(m.triangles.shape), tuple(want_t.shape))
    return m


_FIXTURES = {}


def fixture(N, reso, basis_dim=9):
    """The blob fixture (seeded) of a lattice, its grid, and its mesh at ISO with normals and "sh" colours: made once, shared,
    left unchanged."""
    key = (tuple(reso), basis_dim)
    if key not in _FIXTURES:
        g = MO.blob_fixture(reso, 5 if reso[0] == 17 else 6, basis_dim, radius=(1.0, 0.5, 2.0), center=(0.1, -0.2, 0.3))
        grid = make_grid(N, g)
        _FIXTURES[key] = (g, grid, N.extract_mesh(grid, ISO, world=False))
    return _FIXTURES[key]


# ---- geometry --------------------------------------------------------------------------------------------------------------
def all_cases_grid(rng, iso, empty):
    """2 x 2 x 768: cell z = 3 c carries case c (corner v = 4 di + 2 dj + dk inside iff bit v), the layer between is outside."""
    reso = (2, 2, 768)
    inside = np.zeros(reso, bool)
    for c in range(256):
        for v in range(8):
            inside[(v >> 2) & 1, (v >> 1) & 1, 3 * c + (v & 1)] = (c >> v) & 1
    V = np.where(inside, rng.uniform(iso, 2 * iso, reso), rng.uniform(0.0, 0.999 * iso, reso)).astype(np.float32)
    kept = rng.random(reso) >= empty
    n = int(kept.sum())
    links = np.full(reso, -1, np.int32)
    links[kept] = rng.permutation(n).astype(np.int32)
    density = np.zeros((n, 1), np.float32)
    density[links[kept], 0] = V[kept]
    sh = np.zeros((n, 3), np.float32)
    return {"links": links, "density_data": density, "sh_data": sh, "radius": np.ones(3, np.float32), "center": np.zeros(3, np.float32)}


@pytest.mark.parametrize("empty", [0.0, 0.3])
def test_all_256_cases(N, empty):
    rng = np.random.default_rng(11)
    g = all_cases_grid(rng, ISO, empty)
    if empty == 0.0:      # the lattice does carry every case
        ins = MO.node_values(g["links"], g["density_data"]) >= np.float32(ISO)
        cases = sum(ins[(v >> 2) & 1, (v >> 1) & 1, (v & 1):767 + (v & 1)].astype(int) << v for v in range(8))
        assert set(cases[0::3].tolist()) == set(range(256)) and cases[0::3].tolist() == list(range(256))
    m = assert_geometry_is_the_dense_paths(N, make_grid(N, g), g, ISO)
    assert m.triangles.shape[0] > 500


@pytest.mark.parametrize("reso,seed", [((3, 5, 4), 1), ((2, 7, 2), 2), ((2, 2, 2), 3)])
def test_small_odd_lattices_with_foreign_row_order(N, reso, seed):
    rng = np.random.default_rng(seed)
    for _ in range(4):
        g = MO.random_grid(rng, reso, ISO, empty=0.4)
        kept = g["links"][g["links"] >= 0]
        assert len(set(kept.tolist())) < kept.size < g["density_data"].shape[0]      # a shared row, unreferenced rows
        assert not np.array_equal(kept, np.arange(kept.size))      # not C order
        assert (g["links"] < -1).any() or reso == (2, 2, 2)      # negative links other than -1 (8 nodes may have none)
        assert_geometry_is_the_dense_paths(N, make_grid(N, g), g, ISO)


@pytest.mark.parametrize("reso", [(17, 9, 33), (40, 40, 40)])
def test_tile_edges_on_the_fixture(N, reso):
    """17 x 9 x 33 = 5049 nodes: 3 work tiles of 2048, the last partial; 40^3: 32 tiles."""
    g, grid, mesh = fixture(N, reso)
    m = assert_geometry_is_the_dense_paths(N, grid, g, ISO)
    assert same(m.vertices, mesh.vertices) and same(m.triangles, mesh.triangles)
    assert m.vertices.shape[0] > 500
    # the vertex stage restated in numpy: the same vertices in the same order
    assert cpu(m.vertices).tobytes() == MO.crossing_vertices(MO.node_values(g["links"], g["density_data"]), ISO).tobytes()


def test_axis_limit_lattice(N):
    g = MO.random_grid(np.random.default_rng(4), (2, 2, 1024), ISO, empty=0.4)
    assert_geometry_is_the_dense_paths(N, make_grid(N, g), g, ISO)
    g = MO.random_grid(np.random.default_rng(5), (1024, 2, 2), ISO, empty=0.4)
    assert_geometry_is_the_dense_paths(N, make_grid(N, g), g, ISO)


def test_special_values(N):
    rng = np.random.default_rng(6)
    g = MO.random_grid(rng, (5, 6, 7), ISO, empty=0.2, shared=False)
    d = g["density_data"]
    pick = rng.permutation(d.shape[0])
    d[pick[:20], 0] = np.float32(ISO)      # exactly iso: inside, t = 0
    d[pick[20:40], 0] = np.nan             # outside, t = 0.5
    d[pick[40:55], 0] = np.inf
    d[pick[55:75], 0] = rng.uniform(-50.0, -1.0, 20).astype(np.float32)
    d[pick[75:80], 0] = -np.inf
    m = assert_geometry_is_the_dense_paths(N, make_grid(N, g), g, ISO)
    V = MO.node_values(g["links"], g["density_data"])
    assert cpu(m.vertices).tobytes() == MO.crossing_vertices(V, ISO).tobytes()
    frac = cpu(m.vertices) % 1.0
    assert (frac == 0.5).any() and np.isfinite(cpu(m.vertices)).all()
    # a node at exactly iso next to a (finite or -inf) outside node: t = 0, the vertex sits on the node
    v = set(map(tuple, cpu(m.vertices).tolist()))
    at_iso = np.argwhere((V == np.float32(ISO))[:-1] & (V[1:] < np.float32(ISO)))
    assert len(at_iso) and all(tuple(float(x) for x in q) in v for q in at_iso)


def test_degenerate_grids(N):
    reso = (6, 5, 4)
    n = int(np.prod(reso))
    base = {"radius": np.ones(3, np.float32), "center": np.zeros(3, np.float32), "sh_data": np.zeros((n, 3), np.float32),
            "density_data": np.full((n, 1), 3 * ISO, np.float32)}
    empty = dict(base, links=np.full(reso, -1, np.int32))
    full = dict(base, links=np.arange(n, dtype=np.int32).reshape(reso))
    for g in (empty, full):
        grid = make_grid(N, g)
        for colors in ("sh", "render", None):
            m = N.extract_mesh(grid, ISO, colors=colors)
            assert tuple(m.vertices.shape) == (0, 3) and tuple(m.triangles.shape) == (0, 3)
            assert tuple(m.normals.shape) == (0, 3) and (m.colors is None if colors is None else tuple(m.colors.shape) == (0, 3))
        assert_geometry_is_the_dense_paths(N, grid, g, ISO)
    # no row at all
    none = dict(empty, density_data=np.zeros((0, 1), np.float32), sh_data=np.zeros((0, 3), np.float32))
    assert N.extract_mesh(make_grid(N, none), ISO).triangles.shape[0] == 0


def test_two_calls_return_identical_bytes(N):
    g, grid, mesh = fixture(N, (40, 40, 40))
    again = N.extract_mesh(grid, ISO, world=False)
    for a, b in ((again.vertices, mesh.vertices), (again.triangles, mesh.triangles), (again.normals, mesh.normals),
                 (again.colors, mesh.colors)):
        assert same(a, b)


def test_count_only_and_capacity(N):
    from nerf_projects_amd.grid_mesh import _mc_call
    g, grid, mesh = fixture(N, (17, 9, 33))
    h = grid._handle()
    V, T = mesh.vertices.shape[0], mesh.triangles.shape[0]
    assert _mc_call(grid, h, ISO, None) == (V, T)      # count only: exact
    for dv, dt in ((-1, 0), (0, -1)):
        verts = torch.full((V + dv, 3), -7.0, device="cuda")
        tris = torch.full((T + dt, 3), -7, device="cuda", dtype=torch.int64)
        with pytest.raises(RuntimeError, match="nothing was written"):
            _mc_call(grid, h, ISO, None, verts, tris)
        torch.cuda.synchronize()
        assert (verts == -7.0).all() and (tris == -7).all()
    verts = torch.full((V + 3, 3), -7.0, device="cuda")      # room to spare: only the mesh's rows are written
    tris = torch.full((T + 2, 3), -7, device="cuda", dtype=torch.int64)
    assert _mc_call(grid, h, ISO, None, verts, tris) == (V, T)
    assert same(verts[:V], mesh.vertices) and same(tris[:T], mesh.triangles) and (verts[V:] == -7.0).all() and (tris[T:] == -7).all()
    # only one of the two outputs
    from nerf_projects_amd import _lib
    a = _lib.GridMcArgs()
    n_v, n_t = C.c_int64(), C.c_int64()
    a.iso, a.vertices, a.vertex_capacity, a.n_vertices, a.n_triangles = ISO, verts.data_ptr(), V, C.pointer(n_v), C.pointer(n_t)
    assert grid.ctx.lib.nerf_grid_marching_cubes(h, C.byref(a)) < 0


def test_scratch_is_the_contexts_workspace(N):
    reso = (96, 80, 72)
    n = int(np.prod(reso))
    g = MO.blob_fixture(reso, 9, basis_dim=1, shuffle=False)
    grid = make_grid(N, g)
    N.extract_mesh(grid, ISO, normals=False, colors=None)
    assert grid.ctx.lib.nerf_workspace_bytes(grid.ctx.handle) >= 2 * n      # 2 bytes per node, and a few per 2048


def test_grid_classes_share_the_geometry(N):
    g, grid, mesh = fixture(N, (17, 9, 33))
    for other in (grid.to_half(), grid.to_palette(bits=6), N.BackgroundGrid.from_grid(grid, 2, 8)):
        m = N.extract_mesh(other, ISO, world=False, colors=None)
        assert same(m.vertices, mesh.vertices) and same(m.triangles, mesh.triangles) and same(m.normals, mesh.normals)


def test_world_is_grid2world_of_index(N):
    g, grid, mesh = fixture(N, (17, 9, 33))
    assert g["radius"].tolist() == [1.0, 0.5, 2.0] and g["center"].any()
    w = N.extract_mesh(grid, ISO, world=True, colors=None)
    assert same(w.vertices, grid.grid2world(mesh.vertices)) and same(w.triangles, mesh.triangles)
    assert same(w.normals, mesh.normals)      # normals are world normals in either form
    # node i sits at center - radius + (i + 0.5) 2 radius / reso
    want = g["center"] - g["radius"] + (cpu(mesh.vertices).astype(np.float64) + 0.5) * 2 * g["radius"] / np.array([17, 9, 33])
    assert np.allclose(cpu(w.vertices), want, rtol=0, atol=1e-5)


# ---- mask and components ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("apart,connectivity", [(False, 26), (False, 6), (True, 26), (True, 6)])
def test_largest_component_mask(N, apart, connectivity):
    """The 40^3 fixture at isovalue 30, ``mask=`` the largest component of ``label_components(grid, threshold=30)``: the
    geometry is the dense path's on the masked volume, the mesh is closed, and it has as many connected pieces as the lattice
    says (``expected_surfaces``, scipy). Two things about the fixture, both found on the CPU with ``scipy.ndimage.label``:
      - as its formula stands the two blobs are NOT apart at 30 (``blob_field``: the field between the centres stays above
        41.8), so there the largest component is the whole object; ``apart`` is the same fixture with the second centre moved
        out, where scipy finds two bodies and the mask drops one of them;
      - 26-neighbour components hang together through diagonals that marching cubes separates (the inside corners of an
        ambiguous face are cut apart), so the noisy rim gives such a component a few single-node satellites with surfaces of
        their own; a 6-neighbour component has none, but the 10 % noise leaves it a few enclosed pockets of outside nodes, each
        with a closed surface of its own (2 to 6 of them at every seed tried). Hence the count from the lattice instead of a
        flat 1; with 6 neighbours the mesh is one body's: its outer surface and its pockets' and nothing else."""
    from scipy import ndimage
    iso = 30.0
    g = MO.blob_fixture((40, 40, 40), 6, 1, radius=(1.0, 0.5, 2.0), center=(0.1, -0.2, 0.3), apart=apart)
    grid = make_grid(N, g)
    V = MO.node_values(g["links"], g["density_data"])
    structure = np.ones((3, 3, 3)) if connectivity == 26 else None
    lab, n = ndimage.label(V > np.float32(iso), structure=structure)
    sizes = np.bincount(lab.reshape(-1))[1:]
    assert ndimage.label(MO.blob_field((40, 40, 40), apart) > iso, structure=np.ones((3, 3, 3)))[1] == (2 if apart else 1)
    if apart:      # the separation: two bodies of hundreds of nodes, the rest satellites
        assert np.sort(sizes)[-2] > 500 and (len(sizes) == 2 or np.sort(sizes)[-3] < 10)
    labels, vol = N.label_components(grid, threshold=iso, connectivity=connectivity)
    mask = labels == (vol.argmax() + 1)
    assert np.array_equal(cpu(mask), lab == (np.argmax(sizes) + 1))
    m = assert_geometry_is_the_dense_paths(N, grid, g, iso, mask=mask)
    assert same(N.extract_mesh(grid, iso, mask=mask.to(torch.uint8), world=False, colors=None).vertices, m.vertices)
    tri = cpu(m.triangles)
    assert np.all(MO.edge_counts(tri)[1] == 2)      # closed: every edge in exactly two triangles
    masked = MO.node_values(g["links"], g["density_data"], cpu(mask))
    assert MO.mesh_components(m.vertices.shape[0], tri) == MO.expected_surfaces(masked, iso)
    if connectivity == 6:      # one connected body: its outer surface, and one more around every pocket the noise leaves inside it
        n_inside, n_outside = MO.bodies(masked, iso)
        assert n_inside == 1 and MO.mesh_components(m.vertices.shape[0], tri) == n_outside
    whole = N.extract_mesh(grid, iso, world=False, colors=None)
    assert MO.mesh_components(whole.vertices.shape[0], cpu(whole.triangles)) == MO.expected_surfaces(V, iso)
    assert (whole.triangles.shape[0] > m.triangles.shape[0]) == (apart or connectivity == 6)
    # the masked mesh's normals see the masked values
    n64, bound, _ = MO.normals64(MO.node_values(g["links"], g["density_data"], cpu(mask)), cpu(m.vertices), g["radius"])
    got = cpu(N.mesh_attributes(grid, m.vertices, mask=mask, colors=None)[0])
    ok = bound <= 1e-3
    assert (~ok).sum() <= 0.01 * len(ok) and np.all(np.max(np.abs(got - n64), axis=1)[ok] <= bound[ok])


# ---- normals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reso", [(17, 9, 33), (40, 40, 40)])
def test_normals_against_the_fp64_oracle(N, reso):
    g, grid, mesh = fixture(N, reso)
    pts = cpu(mesh.vertices)
    n64, bound, _ = MO.normals64(MO.node_values(g["links"], g["density_data"]), pts, g["radius"])
    got = cpu(mesh.normals)
    assert got.dtype == np.float32 and got.shape == pts.shape
    ok = bound <= 1e-3      # an ill-conditioned vertex (a vanishing gradient) is left out; at most 1 % may be
    err = np.max(np.abs(got.astype(np.float64) - n64), axis=1)
    print(f"{reso}: {len(ok)} vertices, {int((~ok).sum())} left out, worst error / bound {np.max(err[ok] / bound[ok]):.3f}")
    assert (~ok).sum() <= 0.01 * len(ok)
    assert np.all(err[ok] <= bound[ok]), (np.argmax(err / bound), np.max(err / bound))
    # mesh_attributes at the same points is the same kernel
    again, none = N.mesh_attributes(grid, mesh.vertices, colors=None)
    assert none is None and same(again, mesh.normals)


def winding_dots(grid, mesh, normals):
    tri = cpu(mesh.triangles)
    face = MO.face_normals(cpu(grid.grid2world(mesh.vertices)), tri)
    summed = np.asarray(normals, np.float64)[tri].sum(axis=1)
    dot = np.sum(face * summed, axis=1)
    cos = dot / np.maximum(np.linalg.norm(face, axis=1) * np.linalg.norm(summed, axis=1), 1e-300)
    print(f"{len(tri)} triangles, {int((dot <= 0).sum())} with dot <= 0, least cosine {cos.min():.4f}, median {np.median(cos):.4f}")
    return face, dot, cos


def test_winding_agrees_with_the_normals(N):
    """Every triangle's world face normal has a positive dot product with the sum of its vertex normals: on the 17 x 9 x 33
    fixture (measured: 1 844 triangles, least cosine 0.59) and on the 40^3 lattice with the fixture's field without its noise
    (8 896 triangles, least cosine 0.98).

    On the 40^3 fixture WITH its noise the statement is false of the field itself, not of the kernel: there the noise (10 % of
    about 10, so 1.0 a node) is large against the field's change from node to node (2.7), the surface is rough down to the
    single cell, and the central differences, which look two nodes wide, do not follow every facet. Measured: 231 of 10 968
    triangles have a dot product <= 0 (least cosine -0.998, median 0.96) - and exactly the same 231 with the fp64 oracle's
    normals in place of the kernel's. So that case asserts what can hold: triangle by triangle the sign with the kernel's
    normals is the sign with the oracle's, wherever the oracle's dot product is larger than the normals' rounding bound can move
    it (more than 99 % of the triangles)."""
    g, grid, mesh = fixture(N, (17, 9, 33))
    _, dot, cos = winding_dots(grid, mesh, cpu(mesh.normals))
    assert np.all(dot > 0)
    # the 40^3 lattice, the field without its noise
    reso = (40, 40, 40)
    smooth = MO.blob_fixture(reso, 6, 1, radius=(1.0, 0.5, 2.0), center=(0.1, -0.2, 0.3))
    kept = smooth["links"] >= 0
    smooth["density_data"][smooth["links"][kept], 0] = MO.blob_field(reso)[kept].astype(np.float32)
    sgrid = make_grid(N, smooth)
    smesh = N.extract_mesh(sgrid, ISO, world=False, colors=None)
    _, dot, cos = winding_dots(sgrid, smesh, cpu(smesh.normals))
    assert np.all(dot > 0) and cos.min() > 0.9
    # the 40^3 fixture as it is
    g, grid, mesh = fixture(N, reso)
    n64, bound, _ = MO.normals64(MO.node_values(g["links"], g["density_data"]), cpu(mesh.vertices), g["radius"])
    face, dot, cos = winding_dots(grid, mesh, cpu(mesh.normals))
    _, dot64, _ = winding_dots(grid, mesh, n64)
    slack = np.linalg.norm(face, axis=1) * np.sqrt(3.0) * bound[cpu(mesh.triangles)].sum(axis=1)
    sure = np.abs(dot64) > slack
    assert sure.mean() > 0.99 and np.array_equal(dot[sure] > 0, dot64[sure] > 0)
    assert abs(int((dot <= 0).sum()) - int((dot64 <= 0).sum())) <= int((~sure).sum())


def test_normals_at_arbitrary_points_and_borders(N):
    """A point cloud: points inside cells, on border nodes, outside the lattice (clamped), on a lattice without interior."""
    rng = np.random.default_rng(8)
    for reso in ((17, 9, 33), (2, 3, 2)):
        g = MO.random_grid(rng, reso, ISO, empty=0.3, basis_dim=4)
        grid = make_grid(N, g)
        pts = rng.uniform(-1.5, np.array(reso) + 0.5, (600, 3)).astype(np.float32)
        pts[:50] = np.round(pts[:50])
        pts[50:60] = np.array(reso, np.float32) - 1
        n64, bound, _ = MO.normals64(MO.node_values(g["links"], g["density_data"]), pts, g["radius"])
        got, _ = N.mesh_attributes(grid, gpu(pts), colors=None)
        ok = bound <= 1e-3
        assert ok.mean() > 0.9 and np.all(np.max(np.abs(cpu(got) - n64), axis=1)[ok] <= bound[ok])


def test_zero_gradient_gives_a_zero_normal_and_the_dc_colour(N):
    reso = (4, 4, 4)
    n = 64
    rng = np.random.default_rng(9)
    g = {"links": np.arange(n, dtype=np.int32).reshape(reso), "density_data": np.full((n, 1), 7.0, np.float32),
         "sh_data": rng.normal(0, 0.7, (n, 27)).astype(np.float32), "radius": np.ones(3, np.float32), "center": np.zeros(3, np.float32)}
    grid = make_grid(N, g)
    pts = gpu(rng.uniform(0.0, 3.0, (40, 3)).astype(np.float32))
    normals, sh = N.mesh_attributes(grid, pts, colors="sh")
    _, dc = N.mesh_attributes(grid, pts, colors="dc")
    assert not normals.any() and same(sh, dc)
    S = cpu(grid.sample(pts, grid_coords=True)[1])
    want, bound = MO.colors64(S, 9, "sh", cpu(normals))
    assert np.all(np.abs(cpu(sh) - want) <= bound)


# ---- colours ---------------------------------------------------------------------------------------------------------------
VIEW = (1.0, 2.0, -2.0)


def check_colours(N, grid, pts, normals, basis_dim, mode, got):
    """The oracle is fed the RETURNED normals and the class's own sample rows."""
    S = cpu(grid.sample(pts, grid_coords=True)[1])
    view = (np.array(VIEW) / 3.0).astype(np.float32)
    want, bound = MO.colors64(S, basis_dim, mode, cpu(normals), view)
    got = cpu(got)
    assert got.dtype == np.float32 and got.min() >= 0.0 and got.max() <= 1.0
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err <= bound), (mode, np.max(err / bound))
    return want


@pytest.mark.parametrize("basis_dim", [1, 4, 9])
def test_colours_against_the_fp64_oracle(N, basis_dim):
    g = MO.blob_fixture((17, 9, 33), 5, basis_dim, radius=(1.0, 0.5, 2.0), center=(0.1, -0.2, 0.3))
    rng = np.random.default_rng(basis_dim)
    g["sh_data"] *= rng.choice([0.2, 1.0, 6.0], (g["sh_data"].shape[0], 1)).astype(np.float32)      # both clamps are hit
    grid = make_grid(N, g)
    mesh = N.extract_mesh(grid, ISO, world=False)
    pts, normals = mesh.vertices, mesh.normals
    want = check_colours(N, grid, pts, normals, basis_dim, "sh", mesh.colors)
    assert (want == 0.0).any() and (want == 1.0).any() and ((want > 0.0) & (want < 1.0)).any()
    check_colours(N, grid, pts, normals, basis_dim, "dc", N.extract_mesh(grid, ISO, colors="dc").colors)
    fixed = N.extract_mesh(grid, ISO, colors=VIEW).colors
    check_colours(N, grid, pts, normals, basis_dim, "view", fixed)
    assert same(fixed, N.mesh_attributes(grid, pts, view=VIEW)[1]) and same(fixed, N.mesh_attributes(grid, pts, colors=VIEW)[1])
    assert same(mesh.colors, N.mesh_attributes(grid, pts)[1])
    skipped = N.extract_mesh(grid, ISO, normals=False)      # the colours do not need the normals output
    assert skipped.normals is None and same(skipped.colors, mesh.colors)
    assert N.extract_mesh(grid, ISO, colors=None).colors is None
    if basis_dim == 1:
        assert same(mesh.colors, fixed)


@pytest.mark.parametrize("kind", ["half", "palette", "palette_retain"])
def test_half_and_palette_grids_colour_from_their_own_rows(N, kind):
    g, grid, mesh = fixture(N, (17, 9, 33))
    other = {"half": lambda: grid.to_half(), "palette": lambda: grid.to_palette(bits=6),
             "palette_retain": lambda: grid.to_palette(bits=5, retain=4)}[kind]()
    own = cpu(other.sample(mesh.vertices, grid_coords=True)[1])
    assert not np.array_equal(own, cpu(grid.sample(mesh.vertices, grid_coords=True)[1]))      # its rows are not the fp32 grid's
    for mode, colors in (("sh", "sh"), ("dc", "dc"), ("view", VIEW)):
        normals, got = N.mesh_attributes(other, mesh.vertices, colors=colors)
        assert same(normals, mesh.normals)
        check_colours(N, other, mesh.vertices, normals, 9, mode, got)
    assert not same(N.mesh_attributes(other, mesh.vertices)[1], mesh.colors)


def test_render_colours_are_the_stated_composition(N):
    g, grid, mesh = fixture(N, (17, 9, 33))
    offset = 2.0
    m = N.extract_mesh(grid, ISO, colors="render", world=False, render_offset=offset)
    assert same(m.vertices, mesh.vertices) and same(m.normals, mesh.normals)
    p, n = mesh.vertices, mesh.normals
    scale, _ = grid._affine(p.device)
    n_index = n / scale
    n_index = n_index / n_index.norm(dim=1, keepdim=True)
    assert bool((n != 0).any(dim=1).all())      # (no zero normal on this fixture: the fallback is tested below)
    want = grid.volume_render(N.Rays(grid.grid2world(p + offset * n_index), -n)).clamp(0.0, 1.0)
    assert same(m.colors, want)
    assert float(m.colors.min()) >= 0.0 and float(m.colors.max()) <= 1.0 and float(m.colors.std()) > 0.01
    # a BackgroundGrid renders through its own volume_render
    bg = N.BackgroundGrid.from_grid(grid, 2, 8)
    mb = N.extract_mesh(bg, ISO, colors="render", world=False, render_offset=offset)
    assert same(mb.colors, bg.volume_render(N.Rays(grid.grid2world(p + offset * n_index), -n)).clamp(0.0, 1.0))
    # zero normals take the dc colour
    from nerf_projects_amd.grid_mesh import render_colors
    n0 = n.clone()
    n0[::5] = 0.0
    dc = N.mesh_attributes(grid, p, colors="dc")[1]
    mixed = render_colors(grid, p, n0, dc, offset)
    assert same(mixed[::5], dc[::5]) and torch.isfinite(mixed).all()
    keep = torch.ones(p.shape[0], dtype=torch.bool, device=p.device)
    keep[::5] = False
    assert same(mixed[keep], want[keep])


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_grid_usable(N):
    g, grid, mesh = fixture(N, (17, 9, 33))
    for iso in (0.0, -3.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="isovalue"):
            N.extract_mesh(grid, iso)
    reso = tuple(grid.links.shape)
    ok_mask = torch.ones(reso, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="CPU"):
        N.extract_mesh(grid, ISO, mask=ok_mask.cpu())
    with pytest.raises(RuntimeError, match="CPU"):
        N.mesh_attributes(grid, mesh.vertices.cpu())
    with pytest.raises(ValueError, match="shape of links"):
        N.extract_mesh(grid, ISO, mask=torch.ones((17, 9, 32), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="X, Y, Z"):
        N.extract_mesh(grid, ISO, mask=ok_mask.reshape(-1))
    with pytest.raises(TypeError, match="uint8"):
        N.extract_mesh(grid, ISO, mask=ok_mask.to(torch.float32))
    with pytest.raises(TypeError, match="tensor"):
        N.extract_mesh(grid, ISO, mask=np.ones(reso, np.uint8))
    for colors in ("rgb", 7, (0.0, 0.0, 0.0), (1.0, 2.0)):
        with pytest.raises(ValueError, match="colors"):
            N.extract_mesh(grid, ISO, colors=colors)
    with pytest.raises(ValueError, match="colors"):
        N.mesh_attributes(grid, mesh.vertices, colors="render")
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        N.mesh_attributes(grid, mesh.vertices.reshape(-1))
    # a grid on CPU tensors
    bad = N.SparseGrid.__new__(N.SparseGrid)
    bad._init_common(list(reso), 1.0, 0.0, 1, 9, 0, "cuda")
    bad._links, bad._density, bad._sh = grid.links.cpu(), grid.density_data.cpu(), grid.sh_data.cpu()
    with pytest.raises(RuntimeError, match="CPU"):
        N.extract_mesh(bad, ISO)
    # the C entry refuses on its own, with nothing written
    from nerf_projects_amd import _lib
    from nerf_projects_amd.grid_mesh import _mc_call
    for iso in (0.0, float("nan"), float("inf"), -1.0):
        with pytest.raises(RuntimeError, match="iso"):
            _mc_call(grid, grid._handle(), iso, None)
    a = _lib.GridMeshAttributesArgs()
    out = torch.full((4, 3), -7.0, device="cuda")
    a.points, a.n, a.normals, a.colors = mesh.vertices.data_ptr(), 4, out.data_ptr(), out.data_ptr()
    for mode, view in ((9, (0, 0, 1)), (_lib.NERF_GRID_MESH_COLOR_VIEW, (0, 0, 2)), (_lib.NERF_GRID_MESH_COLOR_NONE, (0, 0, 1))):
        a.color_mode = mode
        a.view[:] = view
        assert grid.ctx.lib.nerf_grid_mesh_attributes(grid._handle(), C.byref(a)) < 0
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    # after all of that the grid extracts what it extracted before
    again = N.extract_mesh(grid, ISO, mask=ok_mask, world=False)
    assert same(again.vertices, mesh.vertices) and same(again.triangles, mesh.triangles) and same(again.colors, mesh.colors)


def test_writers_take_an_extracted_mesh(N, tmp_path):
    g, grid, _ = fixture(N, (17, 9, 33))
    m = N.extract_mesh(grid, ISO)
    m.save_obj(str(tmp_path / "a.obj"))
    N.save_obj(m.vertices, m.triangles, str(tmp_path / "b.obj"), m.colors)
    assert (tmp_path / "a.obj").read_text() == (tmp_path / "b.obj").read_text()
    m.save_ply(str(tmp_path / "a.ply"))
    got = MO.read_ply(str(tmp_path / "a.ply"))
    vert = got["vertex"]
    assert np.stack([vert["x"], vert["y"], vert["z"]], -1).tobytes() == cpu(m.vertices).tobytes()
    assert np.stack([vert["nx"], vert["ny"], vert["nz"]], -1).tobytes() == cpu(m.normals).tobytes()
    assert np.array_equal(np.stack([vert["red"], vert["green"], vert["blue"]], -1), N.to8b(cpu(m.colors)))
    assert np.array_equal(got["face"], cpu(m.triangles))
