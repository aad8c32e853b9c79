"""numpy / torch restatements of the sparse voxel grid's regularisers as values (include/nerf_mi355x.h, "Sparse voxel grid:
regularisers as values"): total variation of a table and the sparsity term of the ray march, each as

  * the fp32 restatement of what csrc/grid_regularisers_kernels.hip computes, every operation a separate fp32 rounding, the
    sums in fp64 (``tv_value``, ``tv_grad``, ``sparsity``, ``sparsity_grad``), and
  * an fp64 torch statement of the same function, differentiated by ``torch.autograd`` (``tv_value64``, ``sparsity64``).

The sparsity term walks its rays in grid_oracle.march, the one sample lattice of the foreground oracles; the fp64 statement
is taken over the sample set that fp32 march shades (the set is piecewise constant in the densities, the sum over it smooth).
A test oracle (not part of the package): slow and simple. A grid is grid_oracle's dict.
"""
import numpy as np
import torch

import grid_oracle as GO

F = GO.F
TV_EPS = 1e-5


def tv_table(g, target):
    """(table [C, cols], ignore_edge) of svox2's tv() / tv_color()"""
    return (g["density_data"], False) if target == "density" else (g["sh_data"], True)


def dense_cells(reso):
    """flat C-order node indices of the (X-1)(Y-1)(Z-1) nodes that have all three forward neighbours, in C order"""
    X, Y, Z = reso
    x, y, z = np.meshgrid(np.arange(X - 1), np.arange(Y - 1), np.arange(Z - 1), indexing="ij")
    return ((x * Y + y) * Z + z).ravel().astype(np.int64)


def _tv_links(links, capacity, cells, edge):
    """per cell of the call: ``live`` (it contributes at all) and the four links 000, +x, +y, +z with anything outside
    [0, capacity), outside the lattice, or of a dead cell as -1"""
    X, Y, Z = links.shape
    cells = np.asarray(cells, np.int64)
    live = (cells >= 0) & (cells < X * Y * Z)
    node = np.where(live, cells, 0)
    z, y, x = node % Z, (node // Z) % Y, node // (Y * Z)
    flat = links.ravel().astype(np.int64)
    own = flat[node]
    if edge:
        live &= own != 0      # the reference's literal `links == 0`
    out = []
    for inside, step in ((np.ones_like(live), 0), (x + 1 < X, Y * Z), (y + 1 < Y, Z), (z + 1 < Z, 1)):
        lk = np.where(inside, flat[np.where(inside, node + step, 0)], -1)
        lk = np.where((lk >= 0) & (lk < capacity) & live, lk, -1)
        out.append(lk)
    return live, out


def _axis_scale(reso, dtype):
    return [dtype(F(s) * F(1.0 / 256.0)) for s in reso]


def _tv_terms(g, target, start_dim, end_dim, cells, dtype=F, table=None):
    """(live [n], links 4 x [n], d 3 x [n, ncol], term [n, ncol]) in ``dtype``, each operation rounded"""
    tab, edge = tv_table(g, target)
    tab = tab if table is None else table
    end_dim = tab.shape[1] if end_dim is None else end_dim
    cells = dense_cells(g["links"].shape) if cells is None else cells
    live, lk = _tv_links(g["links"], tab.shape[0], cells, edge)
    sub = tab[:, start_dim:end_dim].astype(dtype)
    v = [np.where((k >= 0)[:, None], sub[np.maximum(k, 0)], dtype(0.0)) for k in lk]
    if edge:
        v = [v[0]] + [np.where((k >= 0)[:, None], vi, v[0]) for k, vi in zip(lk[1:], v[1:])]
    s = _axis_scale(g["links"].shape, dtype)
    d = [((v[i + 1] - v[0]).astype(dtype) * s[i]).astype(dtype) for i in range(3)]
    ss = dtype(TV_EPS)
    for di in d:
        ss = (ss + (di * di).astype(dtype)).astype(dtype)
    term = np.sqrt(ss).astype(dtype)
    return live, lk, d, term


def tv_value(g, target, start_dim=0, end_dim=None, cells=None):
    """the kernel's value: fp32 terms, summed in fp64, divided by the cell count in fp64, rounded to fp32 once"""
    live, _, _, term = _tv_terms(g, target, start_dim, end_dim, cells)
    n = live.shape[0]
    if n == 0 or term.shape[1] == 0:
        return F(0.0)
    return F(term[live].astype(np.float64).sum() / n)


def tv_grad(g, target, start_dim=0, end_dim=None, cells=None, cotangent=1.0):
    """the kernel's gradient [C, cols] (fp64 sums of the fp32 contributions): w = cotangent / n, each neighbour
    w * ((s_i d_i) / term), the cell w * (-(((s_x dx) + (s_y dy)) + (s_z dz)) / term)"""
    tab, _ = tv_table(g, target)
    end_dim = tab.shape[1] if end_dim is None else end_dim
    out = np.zeros(tab.shape, np.float64)
    live, lk, d, term = _tv_terms(g, target, start_dim, end_dim, cells)
    n = live.shape[0]
    if n == 0 or term.shape[1] == 0:
        return out
    w = F(F(cotangent) / F(n))
    s = _axis_scale(g["links"].shape, F)
    sd = [(s[i] * d[i]).astype(F) for i in range(3)]
    q = [(-((sd[0] + sd[1]).astype(F) + sd[2]).astype(F) / term).astype(F)] + [(sd[i] / term).astype(F) for i in range(3)]
    cols = np.arange(start_dim, end_dim)
    for k, qi in zip(lk, q):
        ok = (k >= 0) & live
        contrib = (w * qi[ok]).astype(F).astype(np.float64)
        np.add.at(out, (k[ok][:, None], cols[None, :]), contrib)
    return out


def tv_value64(g, target, table64, start_dim=0, end_dim=None, cells=None):
    """the same function as an fp64 torch statement of ``table64`` (a [C, cols] fp64 tensor, differentiable): written on
    the lattice of values, independently of ``_tv_terms``"""
    tab, edge = tv_table(g, target)
    end_dim = tab.shape[1] if end_dim is None else end_dim
    links = torch.from_numpy(g["links"].astype(np.int64))
    X, Y, Z = links.shape
    kept = (links >= 0) & (links < tab.shape[0])
    sub = table64[:, start_dim:end_dim]
    lattice = torch.where(kept[..., None], sub[links.clamp(0, max(tab.shape[0] - 1, 0))], torch.zeros((), dtype=torch.float64))
    # one layer of empty nodes beyond the upper faces: a neighbour outside the lattice
    pad = torch.zeros((X + 1, Y + 1, Z + 1, sub.shape[1]), dtype=torch.float64)
    pad[:X, :Y, :Z] = lattice
    kept_pad = torch.zeros((X + 1, Y + 1, Z + 1), dtype=torch.bool)
    kept_pad[:X, :Y, :Z] = kept
    cells = dense_cells((X, Y, Z)) if cells is None else np.asarray(cells, np.int64)
    n = len(cells)
    if n == 0 or sub.shape[1] == 0:
        return torch.zeros((), dtype=torch.float64)
    inside = (cells >= 0) & (cells < X * Y * Z)
    node = cells[inside]
    z, y, x = node % Z, (node // Z) % Y, node // (Y * Z)
    if edge:
        keep = g["links"][x, y, z] != 0
        x, y, z = x[keep], y[keep], z[keep]
    v0 = pad[x, y, z]
    ss = torch.full_like(v0, TV_EPS)
    for i, (ax, ay, az) in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1))):
        vi = pad[x + ax, y + ay, z + az]
        if edge:
            vi = torch.where(kept_pad[x + ax, y + ay, z + az][:, None], vi, v0)
        s = float(F(g["links"].shape[i]) * F(1.0 / 256.0))
        ss = ss + ((vi - v0) * s) ** 2
    return torch.sqrt(ss).sum() / n


def tv_autograd64(g, target, start_dim=0, end_dim=None, cells=None, cotangent=1.0):
    """(value, gradient [C, cols]) of :func:`tv_value64` times ``cotangent`` by fp64 autograd"""
    tab, _ = tv_table(g, target)
    t = torch.from_numpy(tab.astype(np.float64)).requires_grad_(True)
    val = tv_value64(g, target, t, start_dim, end_dim, cells)
    if val.requires_grad:
        (cotangent * val).backward()
    grad = np.zeros(tab.shape) if t.grad is None else t.grad.numpy()
    return float(val.detach()), grad


# ---- the sparsity term -------------------------------------------------------------------------------------------------
def sparsity(g, origins, dirs, step_size=0.5, sigma_thresh=1e-10, stop_thresh=1e-7, near_clip=0.0, skip=None):
    """(s [N] fp32: the kernel's value; s64 [N]: the fp64 sum of log1p(2 sigma^2) over the same samples, sigma the fp32 value;
    shaded-sample count [N]; the sample set: a list of (rays, lk, wa, wb) per pass)"""
    n = len(origins)
    density = g["density_data"]
    step = F(step_size)
    _, _, _, delta_scale, _, _, _ = GO.ray_setup(g, origins, dirs, near_clip)
    s = np.zeros(n, F)
    s64 = np.zeros(n, np.float64)
    count = np.zeros(n, np.int64)
    log_t = np.zeros(n, F)
    samples = []

    def at(rays, t, lk, wa, wb):
        sigma = GO.sigma_at(density, lk, wa, wb)
        hit = sigma > F(sigma_thresh)
        done = np.zeros(rays.size, dtype=bool)
        if hit.any():
            rays, lk, wa, wb, sigma = rays[hit], [k[hit] for k in lk], wa[hit], wb[hit], sigma[hit]
            samples.append((rays, lk, wa, wb))
            s[rays] = (s[rays] + np.log1p((F(2.0) * (sigma * sigma).astype(F)).astype(F)).astype(F)).astype(F)
            s64[rays] += np.log1p(2.0 * sigma.astype(np.float64) ** 2)
            count[rays] += 1
            log_t[rays] = (log_t[rays] + ((-step * sigma).astype(F) * delta_scale[rays]).astype(F)).astype(F)
            done[hit] = np.exp(log_t[rays]).astype(F) < F(stop_thresh)
        return done

    GO.march(g, origins, dirs, at, step_size, near_clip, skip)
    return s, s64, count, samples


def sparsity_grad(g, samples, cotangent):
    """the kernel's gradient [C, 1] over a sample set (fp64 sums of the fp32 contributions):
    d_sigma = g_r * ((4 sigma) / (1 + 2 (sigma sigma))), each kept corner ((w_x w_y) w_z) * d_sigma"""
    density = g["density_data"]
    out = np.zeros(density.shape, np.float64)
    cot = np.asarray(cotangent, F)
    for rays, lk, wa, wb in samples:
        sigma = GO.sigma_at(density, lk, wa, wb)
        d_sigma = (cot[rays] * ((F(4.0) * sigma).astype(F) / (F(1.0) + (F(2.0) * (sigma * sigma).astype(F)).astype(F)).astype(F)).astype(F)).astype(F)
        for c, w8 in GO.corner_weights(wa, wb):
            ok = (lk[c] >= 0) & (lk[c] < density.shape[0])
            np.add.at(out[:, 0], lk[c][ok], (w8[ok] * d_sigma[ok]).astype(F).astype(np.float64))
    return out


def sparsity64(g, samples, density64, n_rays):
    """s [N] as an fp64 torch statement of ``density64`` ([C, 1] fp64 tensor, differentiable) over a fixed sample set"""
    s = torch.zeros(n_rays, dtype=torch.float64)
    cap = density64.shape[0]
    for rays, lk, wa, wb in samples:
        wa64, wb64 = torch.from_numpy(wa.astype(np.float64)), torch.from_numpy(wb.astype(np.float64))
        v = []
        for k in lk:
            kt = torch.from_numpy(k.astype(np.int64))
            ok = (kt >= 0) & (kt < cap)
            v.append(torch.where(ok, density64[kt.clamp(0, max(cap - 1, 0)), 0], torch.zeros((), dtype=torch.float64))[:, None])
        sigma = GO._trilerp(v, wa64, wb64)[:, 0]
        s = s.index_add(0, torch.from_numpy(rays.astype(np.int64)), torch.log1p(2.0 * sigma * sigma))
    return s


def sparsity_autograd64(g, samples, cotangent, n_rays):
    """(s64 [N], gradient [C, 1]) of sum(cotangent * sparsity64) by fp64 autograd"""
    t = torch.from_numpy(g["density_data"].astype(np.float64)).requires_grad_(True)
    s = sparsity64(g, samples, t, n_rays)
    (torch.from_numpy(np.asarray(cotangent, np.float64)) * s).sum().backward()
    return s.detach().numpy(), np.zeros(t.shape) if t.grad is None else t.grad.numpy()
