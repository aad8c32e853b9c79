"""Numpy oracle for the sparse voxel grid's surface meshes (include/nerf_mi355x.h, "Sparse voxel grid: surface meshes").

Geometry needs no oracle of its own: the densified volume (``node_values``) goes through ``marching_cubes_volume``, which
tests/test_mesh.py pins. What is restated here, in fp64 from the same fp32 node values, is the second kernel: the node gradient,
its trilinear interpolation, the world normal, and the colour of an SH row along a direction - each with the a-priori rounding
bound the GPU tests hold the kernel to. ``normals32`` / ``colors32`` restate the kernel's own fp32 operation order; the CPU
tests run them against the fp64 functions so that the bounds are checked without a GPU.
A plain module (no fixtures, no pytest settings).
"""
import numpy as np

U = 2.0 ** -24      # unit roundoff of fp32
SH_C0 = 0.28209479177387814


# ---- fixtures --------------------------------------------------------------------------------------------------------------
def blob_field(reso, apart=False):
    """blob = 60 exp(-4 |x - (0.2, 0.1, -0.3)|^2) + 45 exp(-6 |x + (0.4, 0.3, -0.2)|^2) on the lattice over [-1, 1]^3, fp64.
    The two centres are 0.88 apart and the field between them does not fall below 41.8: at any isovalue that the second blob
    (peak 47.8) survives with its noise, the two are one body. ``apart`` moves the second centre to -(0.6, 0.5, -0.4), 1.22
    from the first: the field between falls to 18.4, and with 10 % noise the blobs are two bodies at isovalue 30."""
    ax = [np.linspace(-1.0, 1.0, n) for n in reso]
    x, y, z = np.meshgrid(*ax, indexing="ij")
    b = (0.6, 0.5, -0.4) if apart else (0.4, 0.3, -0.2)
    return (60.0 * np.exp(-4.0 * ((x - 0.2) ** 2 + (y - 0.1) ** 2 + (z + 0.3) ** 2))
            + 45.0 * np.exp(-6.0 * ((x + b[0]) ** 2 + (y + b[1]) ** 2 + (z + b[2]) ** 2)))


def blob_fixture(reso, seed, basis_dim=9, radius=(1.0, 1.0, 1.0), center=(0.0, 0.0, 0.0), shuffle=True, apart=False):
    """Two noisy Gaussian blobs: v = blob (1 + 0.1 N(0, 1)) with ``blob_field``, nodes with blob <= 2 empty. Rows in a shuffled
    order. Returns the dict ``test_grid.make_grid`` takes."""
    rng = np.random.default_rng(seed)
    blob = blob_field(reso, apart)
    v = blob * (1.0 + 0.1 * rng.standard_normal(reso))
    kept = blob > 2.0
    n = int(kept.sum())
    links = np.full(reso, -1, dtype=np.int32)
    order = rng.permutation(n) if shuffle else np.arange(n)
    links[kept] = order.astype(np.int32)
    density = np.zeros((n, 1), np.float32)
    density[links[kept], 0] = v[kept].astype(np.float32)
    sh = rng.normal(0.0, 0.7, (n, 3 * basis_dim)).astype(np.float32)
    return {"links": links, "density_data": density, "sh_data": sh, "radius": np.asarray(radius, np.float32),
            "center": np.asarray(center, np.float32)}


def random_grid(rng, reso, iso, empty=0.4, basis_dim=1, spare_rows=3, shared=True):
    """Densities uniform in [0, 2 iso], a share ``empty`` of the nodes empty (links -1 or another negative value), rows in a
    shuffled order, ``spare_rows`` rows nobody references and (``shared``) two nodes that name one row."""
    kept = rng.random(reso) >= empty
    n = int(kept.sum())
    rows = n + spare_rows
    links = np.full(reso, -1, dtype=np.int32)
    links[kept] = rng.permutation(rows)[:n].astype(np.int32)
    links[(~kept) & (rng.random(reso) < 0.3)] = -7
    if shared and n >= 2:
        idx = np.flatnonzero(kept.reshape(-1))
        links.reshape(-1)[idx[-1]] = links.reshape(-1)[idx[0]]
    density = rng.uniform(0.0, 2.0 * iso, (rows, 1)).astype(np.float32)
    sh = rng.normal(0.0, 0.7, (rows, 3 * basis_dim)).astype(np.float32)
    return {"links": links, "density_data": density, "sh_data": sh, "radius": np.ones(3, np.float32),
            "center": np.zeros(3, np.float32)}


# ---- node values -----------------------------------------------------------------------------------------------------------
def node_values(links, density, mask=None):
    """The fp32 volume the extraction sees: the row's density where the link is kept and the mask is not 0, else 0."""
    links = np.asarray(links)
    d = np.asarray(density, np.float32).reshape(-1)
    keep = (links >= 0) & (links < d.shape[0])
    if mask is not None:
        keep &= np.asarray(mask) != 0
    if d.shape[0] == 0:
        return np.zeros(links.shape, np.float32)
    return np.where(keep, d[np.clip(links, 0, d.shape[0] - 1)], np.float32(0)).astype(np.float32)


def crossing_vertices(V, iso):
    """The vertex stage of the extraction restated (the header's rule): one vertex per lattice edge whose ends classify
    differently (inside iff v >= iso), at t = (iso - a) / (b - a) in fp32 (0.5 when not finite), ordered by edge key
    3 * node + axis. fp32 ``[n, 3]`` in index coordinates."""
    V = np.asarray(V, np.float32)
    iso = np.float32(iso)
    inside = V >= iso
    X, Y, Z = V.shape
    idx = np.arange(X * Y * Z).reshape(V.shape)
    keys, verts = [], []
    ijk = np.stack(np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij"), -1).astype(np.float32)
    for ax in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        cross = inside[lo] != inside[hi]
        a, b = V[lo][cross], V[hi][cross]
        with np.errstate(all="ignore"):
            t = ((iso - a) / (b - a)).astype(np.float32)
        t = np.where(np.isfinite(t), t, np.float32(0.5)).astype(np.float32)
        p = ijk[lo][cross].copy()
        p[:, ax] = p[:, ax] + t
        keys.append(3 * idx[lo][cross] + ax)
        verts.append(p)
    keys, verts = np.concatenate(keys), np.concatenate(verts)
    return verts[np.argsort(keys, kind="stable")].astype(np.float32)


# ---- the gradient ----------------------------------------------------------------------------------------------------------
def node_gradient(V, dtype=np.float64):
    """G [X, Y, Z, 3]: G_b = h_b (v(q + e_b) - v(q - e_b)), a neighbour outside the lattice replaced by q, h_b = 0.5 in the
    interior and 1 at a border node. In ``dtype`` from the fp32 values (fp32: every operation rounded, as the kernel)."""
    V = np.asarray(V, np.float32).astype(dtype)
    G = np.zeros(V.shape + (3,), dtype)
    for b in range(3):
        n = V.shape[b]
        up = np.take(V, np.minimum(np.arange(n) + 1, n - 1), axis=b)
        dn = np.take(V, np.maximum(np.arange(n) - 1, 0), axis=b)
        h = np.full(n, 0.5, dtype)
        h[0] = h[-1] = 1.0
        shape = [1, 1, 1]
        shape[b] = n
        G[..., b] = h.reshape(shape) * (up - dn)
    return G


def point_cell(points, reso):
    """``(l [N, 3] int, w [N, 3] fp32)``: the sampler's cell and upper weights of fp32 points in index coordinates: clamped
    to [0, reso - 1], l = min(int(x), reso - 2), w = x - l (exact in fp32)."""
    p = np.asarray(points, np.float32)
    hi = np.asarray(reso, np.float32) - 1.0
    with np.errstate(invalid="ignore"):
        p = np.where(np.isnan(p), np.float32(0), np.minimum(np.maximum(p, np.float32(0)), hi)).astype(np.float32)
    l = np.minimum(p.astype(np.int64), np.asarray(reso) - 2)
    return l, (p - l.astype(np.float32)).astype(np.float32)


def trilerp(F, l, w, dtype=np.float64):
    """Trilinear interpolation of the node field F [X, Y, Z, ...] at cells l with upper weights w, in the kernel's order
    (z, then y, then x; lower weight 1 - w). fp32 restates the kernel's roundings, fp64 is the oracle."""
    wb = w.astype(dtype)
    wa = (dtype(1.0) - wb).astype(dtype)
    extra = (1,) * (F.ndim - 3)

    def at(dx, dy, dz):
        return F[l[:, 0] + dx, l[:, 1] + dy, l[:, 2] + dz].astype(dtype)

    def wgt(a, k):
        return a[:, k].reshape((-1,) + extra)

    def lerp(v0, v1, k):
        return (v0 * wgt(wa, k)).astype(dtype) + (v1 * wgt(wb, k)).astype(dtype)
    c00, c01 = lerp(at(0, 0, 0), at(0, 0, 1), 2), lerp(at(0, 1, 0), at(0, 1, 1), 2)
    c10, c11 = lerp(at(1, 0, 0), at(1, 0, 1), 2), lerp(at(1, 1, 0), at(1, 1, 1), 2)
    return lerp(lerp(c00, c01, 1), lerp(c10, c11, 1), 0).astype(dtype)


def world_scale(reso, radius):
    """reso / (2 radius) from the fp32 radius, fp64."""
    return np.asarray(reso, np.float64) / (2.0 * np.asarray(radius, np.float32).astype(np.float64))


def normals64(V, points, radius):
    """``(normal [N, 3], bound [N], gw [N, 3])`` in fp64. ``bound`` is the a-priori bound on ``|n_fp32 - normal|_inf``:
    32 u |A|_2 / |gw|_2 + 16 u, A the interpolation of |G| scaled like gw (inf where gw is 0). The normal is 0 where |gw| is 0
    or not finite."""
    reso = V.shape
    l, w = point_cell(points, reso)
    G = node_gradient(V)
    s = world_scale(reso, radius)
    gw = trilerp(G, l, w) * s
    A = trilerp(np.abs(G), l, w) * s
    norm = np.sqrt(np.sum(gw * gw, axis=1))
    ok = np.isfinite(norm) & (norm > 0)
    with np.errstate(all="ignore"):
        n = np.where(ok[:, None], -gw / norm[:, None], 0.0)
        bound = np.where(ok, 32.0 * U * np.sqrt(np.sum(A * A, axis=1)) / norm + 16.0 * U, np.inf)
    return n, bound, gw


def normals32(V, points, radius, center=(0.0, 0.0, 0.0)):
    """The kernel's own fp32 operation order, restated: for the CPU check of the bound."""
    f = np.float32
    reso = V.shape
    l, w = point_cell(points, reso)
    G = node_gradient(V, np.float32)
    scaling = ((f(0.5) / np.asarray(radius, f)).astype(f) * np.asarray(reso, f)).astype(f)
    gw = (trilerp(G, l, w, np.float32) * scaling).astype(f)
    m = np.max(np.abs(gw), axis=1)
    ok = np.isfinite(m) & (m > 0)
    with np.errstate(all="ignore"):
        s = (gw / m[:, None]).astype(f)
        length = np.sqrt((((s[:, 0] * s[:, 0]).astype(f) + (s[:, 1] * s[:, 1]).astype(f)).astype(f)
                          + (s[:, 2] * s[:, 2]).astype(f)).astype(f)).astype(f)
        n = (-(s / length[:, None])).astype(f)
    return np.where(ok[:, None], n, f(0)).astype(f)


# ---- colours ---------------------------------------------------------------------------------------------------------------
def sh_rows(links, sh, points, dtype=np.float64):
    """S [N, 3 B]: the trilinear interpolation of the rows' coefficients (an empty node is 0) - ``sample``'s."""
    links = np.asarray(links)
    sh = np.asarray(sh, np.float32)
    keep = (links >= 0) & (links < sh.shape[0])
    F = np.where(keep[..., None], sh[np.clip(links, 0, sh.shape[0] - 1)], np.float32(0))
    l, w = point_cell(points, links.shape)
    return trilerp(F, l, w, dtype)


def sh_basis(basis_dim, d):
    """svox2's real SH basis at directions d [N, 3] in d's dtype (fp32: the renderer's operation order)."""
    d = np.asarray(d)
    c = d.dtype.type
    out = np.empty(d.shape[:-1] + (basis_dim,), d.dtype)
    out[..., 0] = c(SH_C0)
    if basis_dim > 1:
        x, y, z = d[..., 0], d[..., 1], d[..., 2]
        out[..., 1] = c(-0.4886025119029199) * y
        out[..., 2] = c(0.4886025119029199) * z
        out[..., 3] = c(-0.4886025119029199) * x
    if basis_dim > 4:
        out[..., 4] = c(1.0925484305920792) * (x * y)
        out[..., 5] = c(-1.0925484305920792) * (y * z)
        out[..., 6] = c(0.31539156525252005) * ((c(2.0) * (z * z) - x * x) - y * y)
        out[..., 7] = c(-1.0925484305920792) * (x * z)
        out[..., 8] = c(0.5462742152960396) * (x * x - y * y)
    return out


def colors64(S, basis_dim, mode, normals=None, view=None):
    """``(rgb [N, 3], bound [N, 3])`` in fp64 from SH rows S [N, 3 B] (the class's own ``sample`` rows) and, for ``"sh"``, the
    RETURNED fp32 normals: clamp(0.5 + sum_k S[c, k] Y_k(d), 0, 1) with d = -normal ("sh"; a zero normal falls back to "dc"),
    d = view ("view") or the constant term alone ("dc"). bound = 2^-19 (0.5 + sum_k |S[c, k]|): 32 roundings of 2^-24 against
    max |Y_k| < 0.64, where the kernel spends about 20."""
    S = np.asarray(S, np.float64).reshape(S.shape[0], 3, basis_dim)
    n = S.shape[0]
    if mode == "dc":
        dc = np.ones(n, bool)
        d = np.zeros((n, 3))
    elif mode == "sh":
        nr = np.asarray(normals, np.float32).astype(np.float64)
        dc = np.all(nr == 0, axis=1)
        d = -nr
    else:
        dc = np.zeros(n, bool)
        d = np.broadcast_to(np.asarray(view, np.float32).astype(np.float64), (n, 3))
    Y = sh_basis(basis_dim, np.ascontiguousarray(d, np.float64))
    Y[dc, 1:] = 0.0
    raw = 0.5 + np.einsum("nck,nk->nc", S, Y)
    used = np.abs(S) * (Y != 0)[:, None, :]
    bound = 2.0 ** -19 * (0.5 + used.sum(axis=2))
    return np.clip(raw, 0.0, 1.0), bound


def colors32(S, basis_dim, mode, normals=None, view=None):
    """The kernel's fp32 operation order restated: the sum in order of k, then 0.5 +, then the clamp."""
    f = np.float32
    S = np.asarray(S, f).reshape(S.shape[0], 3, basis_dim)
    n = S.shape[0]
    if mode == "dc":
        dc, d = np.ones(n, bool), np.zeros((n, 3), f)
    elif mode == "sh":
        nr = np.asarray(normals, f)
        dc, d = np.all(nr == 0, axis=1), (-nr).astype(f)
    else:
        dc, d = np.zeros(n, bool), np.broadcast_to(np.asarray(view, f), (n, 3))
    Y = sh_basis(basis_dim, np.ascontiguousarray(d, f))
    acc = (S[:, :, 0] * Y[:, None, 0]).astype(f)
    full = acc.copy()
    for k in range(1, basis_dim):
        full = (full + (S[:, :, k] * Y[:, None, k]).astype(f)).astype(f)
    acc = np.where(dc[:, None], acc, full)
    return np.clip((f(0.5) + acc).astype(f), f(0), f(1)).astype(f)


# ---- topology --------------------------------------------------------------------------------------------------------------
def edge_counts(triangles):
    """How many triangles use every undirected edge: ``(edges [E, 2], counts [E])``."""
    t = np.asarray(triangles, np.int64)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    e.sort(axis=1)
    return np.unique(e, axis=0, return_counts=True)


def mesh_components(n_vertices, triangles):
    """The number of connected components of the mesh's vertex graph (vertices no triangle uses do not count)."""
    t = np.asarray(triangles, np.int64)
    parent = np.arange(n_vertices)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for a, b in np.concatenate([t[:, [0, 1]], t[:, [1, 2]]]).tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[rb] = ra
    used = np.unique(t)
    return len({find(int(a)) for a in used})


def expected_surfaces(V, iso):
    """How many closed surfaces the isosurface of V has, from the lattice alone (scipy), for a surface that stays off the
    lattice's border. The triangle table is made of the cube's faces alone: on an ambiguous face it cuts the two inside corners
    apart, which joins the two outside ones, and two corners that share only a body diagonal are never joined. So inside nodes
    hang together through lattice edges only (6 neighbours) and outside nodes through edges and face diagonals (18). Every
    closed surface separates one inside body from one outside body, and the bodies with their shared surfaces form a tree:
    surfaces = bodies - 1."""
    n_inside, n_outside = bodies(V, iso)
    return n_inside + n_outside - 1


def bodies(V, iso):
    """``(inside bodies, outside bodies)`` of ``expected_surfaces``: the outside bodies but one are pockets enclosed by the
    inside region."""
    from scipy import ndimage
    inside = np.asarray(V, np.float32) >= np.float32(iso)
    border = np.ones(inside.shape, bool)
    border[1:-1, 1:-1, 1:-1] = False
    assert not (inside & border).any(), "the surface reaches the border of the lattice"
    return ndimage.label(inside)[1], ndimage.label(~inside, structure=ndimage.generate_binary_structure(3, 2))[1]


def face_normals(vertices, triangles):
    """Right-hand normals (not normalised) of the triangles, fp64."""
    v = np.asarray(vertices, np.float64)
    t = np.asarray(triangles, np.int64)
    return np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])


def read_ply(path):
    """A reader for the binary little-endian PLY ``GridMesh.save_ply`` writes: ``{"vertex": structured array, "face": [T, 3]}``
    from the header's own property lists."""
    types = {"float": "<f4", "uchar": "u1", "int": "<i4", "double": "<f8", "uint": "<u4", "short": "<i2", "ushort": "<u2",
             "char": "i1"}
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0", lines[:2]
    elements = []
    for line in lines[2:]:
        tok = line.split()
        if tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            elements[-1][2].append(tok[1:])
    out, off = {}, end
    for name, count, props in elements:
        if name == "vertex":
            dt = np.dtype([(p[1], types[p[0]]) for p in props])
            out["vertex"] = np.frombuffer(data, dt, count, off)
        else:
            assert len(props) == 1 and props[0][0] == "list" and props[0][3] == "vertex_indices", props
            dt = np.dtype([("count", types[props[0][1]]), ("v", types[props[0][2]], 3)])
            f = np.frombuffer(data, dt, count, off)
            assert np.all(f["count"] == 3)
            out["face"] = f["v"]
        off += dt.itemsize * count
    assert off == len(data), "trailing bytes"
    return out
