"""What the sparse voxel grid's size-edge tests share (tests/test_grid_size_edges.py on the GPU, tests/test_grid_size_edges_cpu.py
on the oracle alone) and what tests/test_grid_march.py marches: the hand-made 24^3 grid and its 67 rays, the lattices at the
axis limits of the C ABI (2 and 1024 nodes) with their rays and sample points, and the ray classes the oracle sees on them.
Everything is generated from seeds. A plain module (no fixtures, no pytest settings)."""
import numpy as np

import grid_oracle as GO

RESO = 24
N_RAYS = 67      # 2, 4 or 16 rays per wavefront at basis_dim 9, 4, 1: the last wavefront holds a partial set of groups


def hand_made_grid(basis_dim):
    """24^3 nodes around the origin (node i at (i - 11.5) / 12): a kept ball of radius 8 nodes, dense enough that a ray
    through its middle stops at stop_thresh, and a kept slab two nodes thick on the upper x face, thin enough to see through.
    Rows in random order; empty links are -1 or below."""
    rng = np.random.default_rng(24 + basis_dim)
    i, j, k = np.meshgrid(*(np.arange(RESO, dtype=np.float64),) * 3, indexing="ij")
    r = np.sqrt((i - 11.5) ** 2 + (j - 11.5) ** 2 + (k - 11.5) ** 2)
    ball = r <= 8.0
    slab = np.zeros_like(ball)
    slab[RESO - 2:, 4:20, 4:20] = True
    kept = ball | slab
    n = int(kept.sum())
    links = np.where(rng.uniform(size=kept.shape) < 0.5, -1, -3).astype(np.int32)
    rows = rng.permutation(n).astype(np.int32)
    links[kept] = rows
    density = np.zeros((n, 1), np.float32)
    density[links[ball], 0] = (60.0 * (1.0 - r[ball] / 9.0)).astype(np.float32)      # 60 in the middle, 6.7 at the rim
    density[links[slab & ~ball], 0] = 2.0
    sh = (0.5 * rng.normal(size=(n, 3 * basis_dim))).astype(np.float32)
    return links, density, sh


def hand_made_rays():
    """67 rays, directions not unit: 30 through the ball (9 of them along +x towards it, through the slab), 12 grazing it,
    8 missing the box, 14 starting inside it, one zero direction, one NaN origin, one infinite origin."""
    rng = np.random.default_rng(67)

    def unit(v):
        return v / np.linalg.norm(v, axis=-1, keepdims=True)

    o, d = [], []
    # through the ball: from a sphere of radius 2.5 towards a point within 0.2 of the centre
    src = 2.5 * unit(rng.normal(size=(30, 3)))
    src[:9] = [2.5, 0.0, 0.0] + 0.3 * rng.uniform(-1, 1, (9, 3))
    o.append(src)
    d.append(rng.uniform(-0.2, 0.2, (30, 3)) - src)
    # grazing: past the centre at 0.6 .. 0.72 (the ball's rim is at 8 / 12)
    src = 2.5 * unit(rng.normal(size=(12, 3)))
    side = unit(np.cross(src, rng.normal(size=(12, 3))))
    o.append(src)
    d.append(side * rng.uniform(0.6, 0.72, (12, 1)) - src)
    # missing the box: pointing away from it
    src = 2.5 * unit(rng.normal(size=(8, 3)))
    o.append(src)
    d.append(src + 0.3 * rng.normal(size=(8, 3)))
    # starting inside the box (most of them inside the ball)
    o.append(rng.uniform(-0.9, 0.9, (14, 3)))
    d.append(rng.normal(size=(14, 3)))
    o, d = np.concatenate(o), np.concatenate(d)
    d *= rng.uniform(0.25, 4.0, (len(d), 1))
    o = np.concatenate([o, [[0.1, 0.2, 2.5], [np.nan, 0.0, 2.5], [np.inf, 0.0, 0.0]]])
    d = np.concatenate([d, [[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [-1.0, 0.0, 0.0]]])
    assert o.shape == (N_RAYS, 3) and d.shape == (N_RAYS, 3)
    return o.astype(np.float32), d.astype(np.float32)


def hand_made_dict(basis_dim):
    """:func:`hand_made_grid` as the oracles' grid dict (radius 1, centre 0)"""
    links, density, sh = hand_made_grid(basis_dim)
    return {"links": links, "density_data": density, "sh_data": sh, "radius": np.ones(3, np.float32),
            "center": np.zeros(3, np.float32)}


FIRST_ROW_PAST_2_31 = 79_536_432      # the first row whose entry row * 27 (basis_dim 9) is at or past 2^31: ceil(2^31 / 27)
NAN_FILL = 0x7fc00abc                 # the bits of every float below the linked rows of a large table: a quiet NaN


def large_capacity(n_tail):
    """rows of a table whose last ``n_tail`` rows are the only linked ones and whose first linked entry is past 2^31"""
    return FIRST_ROW_PAST_2_31 + n_tail


# ---- lattices at the axis limits: 2 and 1024 nodes ---------------------------------------------------------------------
EDGE_LATTICES = (((2, 2, 2), 9), ((2, 1024, 3), 9), ((1024, 2, 2), 4), ((3, 2, 1024), 1))      # (reso, basis_dim)
EDGE_RAYS = 96
EDGE_POINTS = 256
BAND = 80


def edge_grid(reso, basis_dim, seed=1):
    """Along the long axis bands of 80 nodes alternate between kept (each node with probability 0.9) and empty, so that the
    skip distances reach their cap of 32 inside an empty band although the other axes are 2 or 3 nodes wide; a 2 x 2 x 2
    lattice keeps each node with probability 0.75. Empty links are -1 or -3, rows in random order, densities U(0, 60), SH
    coefficients 0.5 N(0, 1); radius = reso / max(reso) (cubic cells), centre 0."""
    rng = np.random.default_rng(seed)
    reso = tuple(int(r) for r in reso)
    long_axis = int(np.argmax(reso))
    if max(reso) == 2:
        kept = rng.random(reso) < 0.75
    else:
        shape = [1, 1, 1]
        shape[long_axis] = reso[long_axis]
        band = ((np.arange(reso[long_axis]) // BAND) % 2 == 0).reshape(shape)
        kept = band & (rng.random(reso) < 0.9)
    n = int(kept.sum())
    links = np.where(rng.random(reso) < 0.5, -1, -3).astype(np.int32)
    links[kept] = rng.permutation(n).astype(np.int32)
    density = rng.uniform(0.0, 60.0, (n, 1)).astype(np.float32)
    sh = (0.5 * rng.normal(size=(n, 3 * basis_dim))).astype(np.float32)
    radius = (np.array(reso, np.float64) / max(reso)).astype(np.float32)
    return {"links": links, "density_data": density, "sh_data": sh, "radius": radius, "center": np.zeros(3, np.float32)}


def edge_rays(g, seed=2):
    """96 rays, directions not unit: 48 start inside the box and run along the long axis (either way, tilted by 2e-4), 48 start
    on the sphere of radius 2.5 and aim at a point of the box (some of them at its faces and a little past them)."""
    rng = np.random.default_rng(seed)
    radius = g["radius"].astype(np.float64)
    long_axis = int(np.argmax(g["links"].shape))
    half = EDGE_RAYS // 2
    o1 = rng.uniform(-0.9, 0.9, (half, 3)) * radius
    d1 = 2e-4 * rng.normal(size=(half, 3))
    d1[:, long_axis] += np.where(rng.random(half) < 0.5, -1.0, 1.0)
    u = rng.normal(size=(half, 3))
    o2 = 2.5 * u / np.linalg.norm(u, axis=-1, keepdims=True)
    d2 = rng.uniform(-1.0, 1.0, (half, 3)) * radius - o2
    o, d = np.concatenate([o1, o2]), np.concatenate([d1, d2])
    d *= rng.uniform(0.25, 4.0, (EDGE_RAYS, 1))
    return o.astype(np.float32), d.astype(np.float32)


def edge_points(g, seed=3):
    """256 points in GRID coordinates: 96 inside the box, 64 outside it (up to 3 cells, on any side), 48 exactly on a face
    (-0.5 or size - 0.5 in one or more coordinates), 48 exactly on nodes (the corner nodes of the lattice among them)."""
    rng = np.random.default_rng(seed)
    size = np.array(g["links"].shape, np.float64)
    inside = rng.uniform(-0.5, size - 0.5, (96, 3))
    outside = rng.uniform(-0.5, size - 0.5, (64, 3))
    axis = rng.integers(0, 3, 64)
    outside[np.arange(64), axis] = np.where(rng.random(64) < 0.5, -0.5 - rng.uniform(0.01, 3.0, 64),
                                            size[axis] - 0.5 + rng.uniform(0.01, 3.0, 64))
    faces = rng.uniform(-0.5, size - 0.5, (48, 3))
    on = rng.random((48, 3)) < 0.4
    on[np.arange(48), rng.integers(0, 3, 48)] = True
    faces = np.where(on, np.where(rng.random((48, 3)) < 0.5, -0.5, size - 0.5), faces)
    nodes = np.floor(rng.uniform(0.0, size, (48, 3)))
    nodes[:8] = [[(c >> 2 & 1) * (size[0] - 1), (c >> 1 & 1) * (size[1] - 1), (c & 1) * (size[2] - 1)] for c in range(8)]
    pts = np.concatenate([inside, outside, faces, nodes]).astype(np.float32)
    assert pts.shape == (EDGE_POINTS, 3)
    return pts


def ray_classes(g, o, d):
    """What the oracle sees of rays on a grid at the default options: the rays that stop, end with light left, stay untouched;
    the samples whose links are loaded without and with skip data; the largest skip distance; and whether the render with
    skip data is the render without, bit for bit."""
    skip = GO.skip_distances(g["links"])
    rgb, logt, (visited, shaded) = GO.render(g, o, d, return_counts=True)
    rgb_s, logt_s, (visited_s, shaded_s) = GO.render(g, o, d, skip=skip, return_counts=True)
    return {"stopped": int((logt == np.float32(-1e3)).sum()), "partial": int(((logt < 0) & (logt > -1e3)).sum()),
            "untouched": int((logt == 0).sum()), "visited": visited, "visited_skip": visited_s, "shaded": shaded,
            "shaded_skip": shaded_s, "max_skip": int(skip.max()),
            "same": bool(np.array_equal(rgb, rgb_s) and np.array_equal(logt, logt_s))}
