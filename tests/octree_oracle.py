"""numpy oracle of the PlenOctree (include/nerf_mi355x.h, "PlenOctree"): the build of a tree from a grid's arrays and the
march, vectorised over rays. The traversal (ray set-up, positions, descent, step lengths) runs in ``trav`` - fp32 is the
definition, every numpy operation being one rounded IEEE operation in the order the header writes - and the radiometry
(attenuation, SH sum, activation, accumulation) in ``rad``; ``trav = rad = float64`` is the all-fp64 mode. A plain module."""
import numpy as np

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435)
C4 = (2.5033429417967046, -1.7701307697799304, 0.9461746957575601, -0.6690465435572892, 0.10578554691520431,
      -0.6690465435572892, 0.47308734787878004, -1.7701307697799304, 0.6258357354491761)
MAX_DEPTH = 24


def sh_basis(B, dirs, dtype=np.float64):
    """``[..., B]``: the real SH of degree <= 4 at ``dirs [..., 3]`` in ``dtype``, the header's expressions and order."""
    f = np.dtype(dtype).type
    d = np.asarray(dirs).astype(dtype)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    out = np.empty(d.shape[:-1] + (B,), dtype=dtype)
    out[..., 0] = f(C0)
    if B > 1:
        out[..., 1] = f(-C1) * y
        out[..., 2] = f(C1) * z
        out[..., 3] = f(-C1) * x
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    if B > 4:
        out[..., 4] = f(C2[0]) * xy
        out[..., 5] = f(C2[1]) * yz
        out[..., 6] = f(C2[2]) * ((f(2) * zz - xx) - yy)
        out[..., 7] = f(C2[3]) * xz
        out[..., 8] = f(C2[4]) * (xx - yy)
    if B > 9:
        out[..., 9] = (f(C3[0]) * y) * (f(3) * xx - yy)
        out[..., 10] = (f(C3[1]) * xy) * z
        out[..., 11] = (f(C3[2]) * y) * ((f(4) * zz - xx) - yy)
        out[..., 12] = (f(C3[3]) * z) * ((f(2) * zz - f(3) * xx) - f(3) * yy)
        out[..., 13] = (f(C3[4]) * x) * ((f(4) * zz - xx) - yy)
        out[..., 14] = (f(C3[5]) * z) * (xx - yy)
        out[..., 15] = (f(C3[6]) * x) * (xx - f(3) * yy)
    if B > 16:
        out[..., 16] = (f(C4[0]) * xy) * (xx - yy)
        out[..., 17] = (f(C4[1]) * yz) * (f(3) * xx - yy)
        out[..., 18] = (f(C4[2]) * xy) * (f(7) * zz - f(1))
        out[..., 19] = (f(C4[3]) * yz) * (f(7) * zz - f(3))
        out[..., 20] = f(C4[4]) * (zz * (f(35) * zz - f(30)) + f(3))
        out[..., 21] = (f(C4[5]) * xz) * (f(7) * zz - f(3))
        out[..., 22] = (f(C4[6]) * (xx - yy)) * (f(7) * zz - f(1))
        out[..., 23] = (f(C4[7]) * xz) * (xx - f(3) * yy)
        out[..., 24] = f(C4[8]) * (xx * (xx - f(3) * yy) - yy * (f(3) * xx - yy))
    return out


def measure_depth(child):
    """Depth of the deepest node (root: 0) by a level sweep; ValueError as the package's check."""
    n = child.shape[0]
    flat = child.reshape(n, 8).astype(np.int64)
    if (flat < 0).any() or ((flat > 0) & (np.arange(n)[:, None] + flat >= n)).any():
        raise ValueError("bad child entry")
    frontier, depth = np.zeros(1, np.int64), 0
    while True:
        step = flat[frontier]
        nxt = np.unique((frontier[:, None] + step)[step > 0])
        if nxt.size == 0:
            return depth
        if depth == MAX_DEPTH:
            raise ValueError("too deep")
        depth += 1
        frontier = nxt


def make_tree(child, data, invradius=0.5, offset=0.5, rgb_activation="sigmoid", parent_depth=None):
    child = np.ascontiguousarray(child, dtype=np.int32)
    data = np.ascontiguousarray(data, dtype=np.float32)
    three = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float32), (3,)).copy()      # noqa: E731
    return {"child": child, "data": data, "invradius": three(invradius), "offset": three(offset),
            "rgb_activation": rgb_activation, "max_depth": measure_depth(child),
            "parent_depth": np.zeros((child.shape[0], 2), np.int32) if parent_depth is None else parent_depth}


def build_from_grid(links, density, sh, radius=1.0, center=0.0):
    """svox2's to_svox1 as the header defines the result: ``links [R, R, R]``, ``density [cap, 1]``, ``sh [cap, 3 B]``."""
    links = np.asarray(links)
    R = links.shape[0]
    L = int(np.log2(R))
    assert links.shape == (R, R, R) and 1 << L == R and L >= 1
    D = sh.shape[1] + 1
    occ = {L: links >= 0}
    for l in range(L - 1, 0, -1):
        s = 1 << l
        occ[l] = occ[l + 1].reshape(s, 2, s, 2, s, 2).any(axis=(1, 3, 5))
    coords = {0: np.zeros((1, 3), np.int64)}
    index = {0: np.zeros((1, 1, 1), np.int64)}
    n = 1
    for l in range(1, L):
        coords[l] = np.argwhere(occ[l])      # C order
        index[l] = np.full(occ[l].shape, -1, np.int64)
        index[l][tuple(coords[l].T)] = n + np.arange(len(coords[l]))
        n += len(coords[l])
    child = np.zeros((n, 2, 2, 2), np.int32)
    data = np.zeros((n, 2, 2, 2, D), np.float32)
    parent_depth = np.zeros((n, 2), np.int32)
    for l in range(L):
        own = index[l][tuple(coords[l].T)]
        if l > 0:
            par = index[l - 1][tuple((coords[l] >> 1).T)]
            bits = coords[l] & 1
            parent_depth[own, 0] = par * 8 + bits[:, 0] * 4 + bits[:, 1] * 2 + bits[:, 2]
            parent_depth[own, 1] = l
        for u in range(2):
            for v in range(2):
                for w in range(2):
                    cc = coords[l] * 2 + np.array([u, v, w])
                    if l + 1 < L:
                        ci = index[l + 1][tuple(cc.T)]
                        child[own, u, v, w] = np.where(ci >= 0, ci - own, 0)
                    else:
                        lk = links[tuple(cc.T)]
                        kept = lk >= 0
                        data[own[kept], u, v, w, :-1] = sh[lk[kept]]
                        data[own[kept], u, v, w, -1] = density[lk[kept], 0]
    r = np.broadcast_to(np.asarray(radius, np.float32), (3,))
    c = np.broadcast_to(np.asarray(center, np.float32), (3,))
    return make_tree(child, data, np.float32(0.5) / r, np.float32(0.5) * (np.float32(1.0) - c / r), "relu_half", parent_depth)


def _unit(p, inv, f):
    """unit(p) of the header; fmin / fmax drop a NaN as the device's do."""
    t1 = -p * inv
    t2 = t1 + inv
    lo, hi = np.fmin(t1, t2), np.fmax(t1, t2)
    tmin = np.fmax(np.fmax(np.fmax(f(0), lo[..., 0]), lo[..., 1]), lo[..., 2])
    tmax = np.fmin(np.fmin(np.fmin(f(np.float32(1e9)), hi[..., 0]), hi[..., 1]), hi[..., 2])
    return tmin, tmax


def march(tree, origins, dirs, step_size=1e-3, sigma_thresh=0.0, stop_thresh=0.0, background_brightness=1.0,
          trav=np.float32, rad=np.float32, max_iters=1 << 16):
    """``(rgb [n, 3] in rad, steps [n] int32, leaves [n, max steps] int64 cell indices padded with -1)``."""
    f, r = np.dtype(trav).type, np.dtype(rad).type
    k = lambda v: f(np.float32(v))      # noqa: E731  (the fp32 constants, widened in the fp64 mode)
    child = tree["child"].reshape(-1).astype(np.int64)
    D = tree["data"].shape[-1]
    B = (D - 1) // 3
    data = tree["data"].reshape(-1, D)
    relu_half = tree["rgb_activation"] == "relu_half"
    ow = np.asarray(origins, np.float32)
    dw = np.asarray(dirs, np.float32)
    n = ow.shape[0]
    step = k(step_size)
    with np.errstate(all="ignore"):
        o = ow.astype(trav) * tree["invradius"].astype(trav) + tree["offset"].astype(trav)
        d = dw.astype(trav) * tree["invradius"].astype(trav)
        ds = f(1) / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        d = d * ds[:, None]
        inv = f(1) / (d + k(1e-9))
        ok = np.isfinite(ow).all(1) & np.isfinite(dw).all(1) & np.isfinite(ds) & (ds > 0)
        tmin, tmax = _unit(o, inv, f)
        basis = sh_basis(B, dw, rad)
        hi = f(np.float32(1.0) - np.float32(1e-6))
        active = ok & ~(tmax < 0) & ~(tmin > tmax)
        t = tmin.copy()
        T = np.ones(n, rad)
        rgb = np.zeros((n, 3), rad)
        steps = np.zeros(n, np.int32)
        done = np.zeros(n, bool)
        leaves = []
        for it in range(max_iters):
            active = active & (t < tmax)
            idx = np.nonzero(active)[0]
            if idx.size == 0:
                break
            steps[idx] += 1
            p = np.fmin(np.fmax(o[idx] + t[idx, None] * d[idx], f(0)), hi)
            node = np.zeros(idx.size, np.int64)
            cell = np.zeros(idx.size, np.int64)
            inv_cube = np.ones(idx.size, trav)
            live = np.ones(idx.size, bool)
            for _ in range(tree["max_depth"] + 1):
                p2 = p * f(2)
                u = (p2 >= f(1)).astype(np.int64)
                p = np.where(live[:, None], p2 - u.astype(trav), p)
                inv_cube = np.where(live, inv_cube * f(0.5), inv_cube)
                cell = np.where(live, node * 8 + u[:, 0] * 4 + u[:, 1] * 2 + u[:, 2], cell)
                skip = child[cell]
                live = live & (skip != 0)
                node = np.where(live, node + skip, node)
                if not live.any():
                    break
            col = np.full(n, -1, np.int64)
            col[idx] = cell
            leaves.append(col)
            a, b = _unit(p, inv[idx], f)
            delta = (b - a) * inv_cube + step
            row = data[cell]
            sigma32 = row[:, D - 1]
            shade = sigma32 > np.float32(sigma_thresh)
            if shade.any():
                j = idx[shade]
                rw = row[shade].astype(rad)
                att = np.exp((-delta[shade].astype(rad) * ds[j].astype(rad)) * rw[:, D - 1])
                weight = T[j] * (r(1) - att)
                for c in range(3):
                    s = basis[j, 0] * rw[:, c * B]
                    for i in range(1, B):
                        s = s + basis[j, i] * rw[:, c * B + i]
                    colour = np.maximum(s + r(0.5), r(0)) if relu_half else r(1) / (r(1) + np.exp(-s))
                    rgb[j, c] = rgb[j, c] + weight * colour
                T[j] = T[j] * att
                stopped = j[T[j] <= r(np.float32(stop_thresh))]
                if stopped.size:
                    rgb[stopped] = rgb[stopped] * (r(1) / (r(1) - T[stopped]))[:, None]
                    done[stopped] = True
                    active[stopped] = False
            tn = t[idx] + delta
            adv = tn > t[idx]
            active[idx[~adv]] = False
            t[idx] = np.where(adv, tn, t[idx])
        else:
            raise AssertionError("a ray reached the cap of the march")
        add_bg = ok & ~done
        rgb[add_bg] = rgb[add_bg] + (T[add_bg] * r(np.float32(background_brightness)))[:, None]
        rgb[~ok] = np.nan
    lv = np.stack(leaves, 1) if leaves else np.zeros((n, 0), np.int64)
    # a ray's leaves in the order it visited them (columns are march passes; a ray is active in a prefix of them)
    return rgb, steps, lv


# ---- the cases test_octree_cpu.py and test_octree.py share -----------------------------------------------------------------
def fixture_grid(seed, R, B, kind="random", keep=0.3):
    """``(links [R, R, R] int32, density [cap, 1], sh [cap, 3 B])`` fp32, seeded. kind: "random" (a fraction ``keep`` of the
    nodes, rows in a shuffled order), "octants" (octant 0 empty, octant 7 full, the rest random), "single" (one kept node)."""
    rng = np.random.default_rng(seed)
    kept = rng.random((R, R, R)) < keep
    h = R // 2
    if kind == "octants":
        kept[:h, :h, :h] = False
        kept[h:, h:, h:] = True
    elif kind == "single":
        kept[:] = False
        kept[tuple(rng.integers(0, R, 3))] = True
    cap = int(kept.sum())
    links = np.full((R, R, R), -1, np.int32)
    links[kept] = rng.permutation(cap).astype(np.int32)
    links[(~kept) & (rng.random((R, R, R)) < 0.1)] = -3      # any negative value is empty
    density = (np.minimum(rng.gamma(1.0, 2.0, (cap, 1)), 4.0) * (rng.random((cap, 1)) < 0.9)).astype(np.float32)
    sh = (rng.standard_normal((cap, 3 * B)) * (0.8 / np.sqrt(B))).astype(np.float32)
    return links, density, sh


def fixture_rays(seed, n, radius=1.0, center=0.0):
    """``(origins, dirs) [n, 3]`` fp32: seeded rays from a shell around the box towards points in it (unit directions), the
    last ones replaced by: a miss, a ray grazing the face x = radius, one starting inside, two along axes (zero components),
    one with a non-unit direction, one NaN ray."""
    rng = np.random.default_rng(seed)
    c = np.broadcast_to(np.asarray(center, np.float64), (3,))
    v = rng.standard_normal((n, 3))
    o = c + v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(1.75, 2.2, (n, 1)) * radius
    target = c + rng.uniform(-0.9, 0.9, (n, 3)) * radius
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o[-7], d[-7] = c + [3.0 * radius, 0.0, 0.0], [0.0, 1.0, 0.0]                          # a miss
    o[-6], d[-6] = c + [radius, -2.0 * radius, 0.13 * radius], [0.0, 1.0, 0.0]            # grazes a face
    o[-5], d[-5] = c + [0.11 * radius, -0.23 * radius, 0.31 * radius], d[0]                # starts inside
    o[-4], d[-4] = c + [-2.0 * radius, 0.37 * radius, -0.41 * radius], [1.0, 0.0, 0.0]     # along x
    o[-3], d[-3] = c + [0.21 * radius, 0.17 * radius, 2.5 * radius], [0.0, 0.0, -1.0]      # along -z
    d[-2] = d[-2] * 1.25                                                                   # not unit
    o, d = o.astype(np.float32), d.astype(np.float32)
    o[-1, 1] = np.nan
    return o, d


# name: (R, basis_dim, kind, seed, rays). Seeds chosen (and asserted in test_octree_cpu.py) so that the fp32 and the all-fp64
# traversal visit the same leaves on >= 99 % of the rays and agree there within the GPU tests' bar.
CASES = {
    "r2": (2, 1, "random", 1, 512),
    "r8": (8, 4, "octants", 1, 1024),
    "r16": (16, 9, "random", 2, 1024),
    "single": (16, 1, "single", 1, 512),
    "sh16": (16, 16, "random", 2, 1024),
    "sh25": (16, 25, "random", 2, 1024),
}
_case_cache = {}


def case(name):
    """``(grid arrays, tree, origins, dirs)`` of a case, computed once and shared (do not write into them)."""
    if name not in _case_cache:
        R, B, kind, seed, n = CASES[name]
        grid = fixture_grid(seed, R, B, kind)
        _case_cache[name] = (grid, build_from_grid(*grid), *fixture_rays(100 + seed, n))
    return _case_cache[name]


def same_leaves(la, lb):
    """Per ray: did two marches visit the same leaf sequence."""
    w = max(la.shape[1], lb.shape[1])
    pad = lambda a: np.pad(a, ((0, 0), (0, w - a.shape[1])), constant_values=-1)      # noqa: E731
    return (pad(la) == pad(lb)).all(1)


def with_activation(tree, act):
    t = dict(tree)
    t["rgb_activation"] = act
    return t
