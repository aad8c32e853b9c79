"""numpy restatement of sparse-voxel-grid resampling (include/nerf_mi355x.h, "Sparse voxel grid: resampling").

It states what ``resample_grid`` computes - the lattice, the trilinear sample of the old grid at every node, the threshold,
the dilation, links as the running index over kept nodes, the gather of the new tables - and the weight render, with every
operation a separate rounding in ``dtype`` (fp32 mirrors the kernels operation by operation; fp64 is the same statement in
double, for the weight render on the fp32 statement's own positions and cells). A test oracle, not part of the package: slow
and simple. A grid is a dict as in tests/grid_oracle.py.
"""
import numpy as np

import grid_oracle as GO

F = np.float32


def lattice_axes(old_reso, reso):
    """svox2's lattice: torch.linspace(f - 0.5, R - f - 0.5, R') with f = 0.5 R / R', fp32 (the host computes it with torch,
    as the reference does; it arrives at the kernels as data)."""
    import torch
    out = []
    for r_old, r_new in zip(old_reso, reso):
        f = 0.5 * r_old / r_new
        out.append(torch.linspace(f - 0.5, r_old - f - 0.5, r_new, dtype=torch.float32).numpy())
    return out


def _cell(p, size, dtype):
    """clamped coordinate -> base cell and upper weight, along one axis"""
    p = np.minimum(np.maximum(p.astype(dtype), dtype(0.0)), dtype(size - 1))
    l = np.minimum(p.astype(np.int64), size - 2)
    return l, (p - l.astype(dtype)).astype(dtype)


def _trilerp(v, wa, wb):
    """v: 8 arrays [n, C] in corner order 000, 001, ..., 111 (x, y, z bits); wa, wb: 3 arrays [n, 1]; z, then y, then x"""
    c00 = v[0] * wa[2] + v[1] * wb[2]
    c01 = v[2] * wa[2] + v[3] * wb[2]
    c10 = v[4] * wa[2] + v[5] * wb[2]
    c11 = v[6] * wa[2] + v[7] * wb[2]
    c0 = c00 * wa[1] + c01 * wb[1]
    c1 = c10 * wa[1] + c11 * wb[1]
    return c0 * wa[0] + c1 * wb[0]


def _fetch(links, table, dtype):
    cap = table.shape[0]
    ok = (links >= 0) & (links < cap)
    out = np.zeros((links.shape[0], table.shape[1]), dtype=dtype)
    out[ok] = table[links[ok]].astype(dtype)
    return out


def sample_nodes(grid, axes, nodes, table, dtype=F):
    """``table`` of ``grid`` interpolated at the lattice nodes ``nodes`` (flat C-order indices into the lattice of ``axes``)"""
    links = grid["links"]
    reso = [len(a) for a in axes]
    idx = np.unravel_index(nodes, reso)
    l, wa, wb = [], [], []
    for k in range(3):
        lk, w = _cell(np.asarray(axes[k], F)[idx[k]], links.shape[k], dtype)
        l.append(lk)
        wb.append(w[:, None])
        wa.append((dtype(1.0) - w).astype(dtype)[:, None])
    v = []
    for c in range(8):
        v.append(_fetch(links[l[0] + ((c >> 2) & 1), l[1] + ((c >> 1) & 1), l[2] + (c & 1)], table, dtype))
    out = _trilerp(v, wa, wb)
    assert out.dtype == dtype
    return out


def lattice_density(grid, axes, dtype=F):
    reso = [len(a) for a in axes]
    n = reso[0] * reso[1] * reso[2]
    return sample_nodes(grid, axes, np.arange(n), grid["density_data"], dtype)[:, 0].reshape(reso)


def dilate(mask):
    """one step of the 27-neighbourhood OR, indices clamped at the faces"""
    m = np.pad(np.asarray(mask) != 0, 1, mode="edge")
    X, Y, Z = mask.shape
    out = np.zeros(mask.shape, dtype=bool)
    for a in range(3):
        for b in range(3):
            for c in range(3):
                out |= m[a:a + X, b:b + Y, c:c + Z]
    return out


def links_of(mask):
    flat = np.asarray(mask).reshape(-1) != 0
    links = np.cumsum(flat, dtype=np.int64) - 1
    links[~flat] = -1
    return links.astype(np.int32).reshape(mask.shape)


def lattice_consts(reso, radius, center):
    """offset, scaling of a grid of ``reso`` as nerf_grid_create computes them"""
    gsz = np.array(reso, dtype=F)
    radius, center = np.asarray(radius, F), np.asarray(center, F)
    offset = ((F(0.5) * (F(1.0) - center / radius)).astype(F) * gsz).astype(F) - F(0.5)
    scaling = ((F(0.5) / radius).astype(F) * gsz).astype(F)
    return offset.astype(F), scaling.astype(F)


def weight_render(volume, cam, radius, center, step_size=0.5, stop_thresh=0.2, dtype=F, out=None):
    """The max-weight volume of one camera ``cam`` = dict(c2w, fx, fy, cx, cy, width, height). Positions, cells and trilinear
    weights are the fp32 ones of the header in both dtypes; sigma, the exponentials, the weight and log T are in ``dtype``.
    Returns ``out`` (float array of ``dtype``, raised in place when given)."""
    vol = np.asarray(volume)
    reso = vol.shape
    if out is None:
        out = np.zeros(reso, dtype=dtype)
    origins, dirs = GO.gen_rays(cam["c2w"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["width"], cam["height"])
    offset, scaling = lattice_consts(reso, radius, center)
    step = F(step_size)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = dirs.astype(F)
        dn = np.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(F) + d[:, 2] * d[:, 2]).astype(F)).astype(F)
        o = (offset + (origins.astype(F) * scaling).astype(F)).astype(F)
        g = ((d / dn[:, None]).astype(F) * scaling).astype(F)
        delta_scale = (F(1.0) / np.sqrt(((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]).astype(F) + g[:, 2] * g[:, 2]).astype(F)).astype(F)).astype(F)
        world_step = (delta_scale * step).astype(F)
        g = (g * delta_scale[:, None]).astype(F)
        inv = (F(1.0) / g).astype(F)
        gsz = np.array(reso, dtype=F)
        t1 = ((F(-0.5) - o).astype(F) * inv).astype(F)
        t2 = (((gsz - F(0.5)).astype(F) - o).astype(F) * inv).astype(F)
        lo, hi = np.fmin(t1, t2), np.fmax(t1, t2)
        t = np.zeros(o.shape[0], dtype=F)
        tmax = np.full(o.shape[0], F(2e3), dtype=F)
        for k in range(3):
            use = g[:, k] != 0
            t = np.where(use, np.fmax(t, lo[:, k]), t).astype(F)
            tmax = np.where(use, np.fmin(tmax, hi[:, k]), tmax).astype(F)
        ok = (dn > 0) & np.isfinite(dn) & np.isfinite(delta_scale) & np.isfinite(o).all(-1) & np.isfinite(g).all(-1) \
            & np.isfinite(t) & (t <= tmax)
    act = np.nonzero(ok)[0]
    log_t = np.zeros(o.shape[0], dtype=dtype)
    flat = out.reshape(-1)
    volf = vol.reshape(-1).astype(dtype)
    s0, s1 = reso[1] * reso[2], reso[2]
    while act.size:
        t_next = (t[act] + step).astype(F)
        act, t_next = act[t_next > t[act]], t_next[t_next > t[act]]
        if not act.size:
            break
        l, wa, wb = [], [], []
        for k in range(3):
            lk, w = _cell((o[act, k] + (t[act] * g[act, k]).astype(F)).astype(F), reso[k], F)
            l.append(lk)
            wb.append(w.astype(dtype)[:, None])
            wa.append((F(1.0) - w).astype(F).astype(dtype)[:, None])
        base = (l[0] * reso[1] + l[1]) * reso[2] + l[2]
        corners = [base + ((c >> 2) & 1) * s0 + ((c >> 1) & 1) * s1 + (c & 1) for c in range(8)]
        sigma = _trilerp([volf[c][:, None] for c in corners], wa, wb)[:, 0]
        assert sigma.dtype == dtype
        hit = sigma > dtype(F(1e-8))
        stopped = np.zeros(act.size, dtype=bool)
        if hit.any():
            rays = act[hit]
            log_att = ((-world_step[rays]).astype(dtype) * sigma[hit]).astype(dtype)
            weight = (np.exp(log_t[rays]).astype(dtype) * (dtype(1.0) - np.exp(log_att).astype(dtype))).astype(dtype)
            log_t[rays] = (log_t[rays] + log_att).astype(dtype)
            for c in corners:
                np.maximum.at(flat, c[hit], weight)
            stopped[hit] = np.exp(log_t[rays]).astype(dtype) < dtype(F(stop_thresh))
        t[act] = t_next
        act = act[~stopped & (t[act] <= tmax[act])]
    return out


def resample(grid, reso, sigma_thresh=5.0, weight_thresh=0.01, dilate_steps=2, cameras=None, weight_render_stop_thresh=0.2,
             dtype=F):
    """The whole of resample_grid (without max_elements): dict with links, density_data, sh_data of the new grid, and mask
    (before dilation: what the threshold decided), volume (the lattice density) and, with cameras, max_weight."""
    reso = [int(reso)] * 3 if np.isscalar(reso) else [int(r) for r in reso]
    axes = lattice_axes(grid["links"].shape, reso)
    volume = lattice_density(grid, axes, dtype)
    out = {"volume": volume, "axes": axes}
    if cameras is not None:
        maxw = np.zeros(reso, dtype=dtype)
        for cam in cameras:
            weight_render(volume, cam, grid["radius"], grid["center"], 0.5, weight_render_stop_thresh, dtype, out=maxw)
        out["max_weight"] = maxw
        mask = maxw >= dtype(F(weight_thresh))
    else:
        mask = volume >= dtype(F(sigma_thresh))
    out["mask"] = mask.copy()
    for _ in range(int(dilate_steps)):
        mask = dilate(mask)
    links = links_of(mask)
    nodes = np.nonzero(mask.reshape(-1))[0]
    out["links"] = links
    out["density_data"] = volume.reshape(-1)[nodes].reshape(-1, 1)
    out["sh_data"] = sample_nodes(grid, axes, nodes, grid["sh_data"], dtype) if nodes.size else \
        np.zeros((0, grid["sh_data"].shape[1]), dtype=dtype)
    out["radius"], out["center"] = np.asarray(grid["radius"], F), np.asarray(grid["center"], F)
    return out


# ---- the recorded reference (tests/golden/grid_resample.npz) --------------------------------------------------------------
EXACT_CASES = ("b_x2", "c_x2", "a_same", "c_same")      # 2x (weights are quarters, every product exact) and the same lattice


def fixture_cases(z):
    return [(str(c), str(s), [int(r) for r in reso], float(t))
            for c, s, reso, t in zip(z["cases"], z["sources"], z["resos"], z["sigma_thresh"])]


def check_against_fixture(got, z, case, grid, reso, thresh, who):
    """``got`` (dict with links, density_data, sh_data as numpy) against the reference's recorded resample of ``grid``.
    Values are compared per node through ``links``, never by row: one mask flip renumbers every later row. Nodes kept by both
    must agree within max(3 d_ref, 1e-5 max|.|); the mask may differ from the reference's fp64 mask only at nodes whose fp64
    density is within that bar of the threshold, and at no more than 1e-3 of the lattice. The 2x and same-resolution cases
    are bit-equal. Returns the figures."""
    l_ref, d_ref_t, s_ref_t = z[f"{case}_links"], z[f"{case}_density"], z[f"{case}_sh"]
    n = l_ref.size
    assert list(got["links"].shape) == list(l_ref.shape) == list(reso)
    assert got["links"].dtype == np.int32 and got["density_data"].dtype == F and got["sh_data"].dtype == F
    m64 = np.unpackbits(z[f"{case}_mask64"])[:n].astype(bool).reshape(l_ref.shape)
    m_got, m_ref = got["links"] >= 0, l_ref >= 0
    assert np.array_equal(np.sort(got["links"][m_got]), np.arange(int(m_got.sum())))      # a numbering of the kept nodes
    assert got["density_data"].shape == (int(m_got.sum()), 1) and got["sh_data"].shape == (int(m_got.sum()), s_ref_t.shape[1])
    d_ref = z[f"{case}_d_ref"]
    bar_d = max(3.0 * float(d_ref[0]), 1e-5 * float(np.abs(d_ref_t).max()))
    bar_s = max(3.0 * float(d_ref[1]), 1e-5 * float(np.abs(s_ref_t).max()))
    both = m_got & m_ref
    err_d = np.abs(got["density_data"][got["links"][both]].astype(np.float64) - d_ref_t[l_ref[both]])
    err_s = np.abs(got["sh_data"][got["links"][both]].astype(np.float64) - s_ref_t[l_ref[both]])
    vol64 = lattice_density(grid, lattice_axes(grid["links"].shape, reso), np.float64)
    assert np.array_equal(vol64 >= thresh, m64), "the fp64 restatement and the reference's fp64 run disagree on the mask"
    flips = m_got != m64
    fig = {"kept": int(m_got.sum()), "nodes": n, "err_density": float(err_d.max()) if err_d.size else 0.0, "bar_density": bar_d,
           "err_sh": float(err_s.max()) if err_s.size else 0.0, "bar_sh": bar_s, "flips": int(flips.sum())}
    print(f"{who} {case}: kept {fig['kept']} of {n}; density err {fig['err_density']:.3e} (bar {bar_d:.3e}), sh err "
          f"{fig['err_sh']:.3e} (bar {bar_s:.3e}); mask flips vs fp64 {fig['flips']}")
    assert both.sum() > 0
    assert fig["err_density"] <= bar_d and fig["err_sh"] <= bar_s, fig
    assert (np.abs(vol64[flips] - thresh) <= bar_d).all(), fig
    assert fig["flips"] <= 1e-3 * n, fig
    if case in EXACT_CASES:
        assert np.array_equal(got["links"], l_ref), case
        assert np.array_equal(got["density_data"], d_ref_t) and np.array_equal(got["sh_data"], s_ref_t), case
    return fig
