"""Writes tests/golden/grid_background_train.npz: autograd gradients of the MSE loss of the composite render (foreground, then
background layers) with respect to ``density_data``, ``sh_data`` and ``background_data``, in fp64 and in fp32, and a short
RMSProp loop on all three tables.

    NERF_REFERENCE_SVOX2=/path/to/reference/svox2 python tests/golden/make_golden_grid_background_train.py

Runs on the CPU. Nothing of the reference is copied: the fixture holds arrays only.

The foreground comes by the route of make_golden_grid_train.py: PyTorch autograd through the reference's
``SparseGrid._volume_render_gradcheck_lerp`` (the CUDA semantics at ``sigma_thresh = 0``, ``stop_thresh = 0``), whose final
transmittance ``exp(log_T)`` is taken where the renderer multiplies it by ``background_brightness``. The background is a torch
transcription of the forward stated in include/nerf_mi355x.h, "Sparse voxel grid: background layers" (the reference's CUDA
kernel, which cannot run here): its geometry is the reference's ``ConcentricSpheresIntersector`` / ``xyz2equirect`` on the
foreground set-up's fp32 ``o``, ``d``, ``delta_scale``, as make_golden_grid_background.py takes it. Both run once on fp32 and
once on fp64 tensors; ``d_ref`` = max |fp32 gradient - fp64 gradient| per table.

The shapes are those of grid_background.npz: foreground (12, 14, 10), R = 8 with L = 2, 5, 8, a quarter of the texels without
a row, rows permuted, sigma in [-1, 6], 512 rays of its kinds, step_size 0.5 / 0.3, stop_thresh 1e-7 / 0.05, brightness 1 / 0.
The reference's renderer has no stop rule, the kernels' foreground has: the foreground made here is light (a ray keeps
exp(log_T) > 0.05 through it) except for a few very dense nodes, and a ray whose log_T after any foreground sample lies in
[-25, log(0.05) + 0.05] is drawn again - so a ray either never stops in the foreground or stops where nothing behind it
counts (below e^-25), and the two statements agree. Asserted on the output: the coverage counts printed at the end.

The loop: 20 iterations of 256 rays towards the recorded fp64 render of one setting, from half the light densities, zero SH
and half the background, masked RMSProp as include/nerf_mi355x.h states it on the rows and (row, layer) entries a step
touches - svox2's masks, which are set whatever the gradient: an entry whose weight is exactly zero (w_z = 0 on the innermost
spheres) is stepped with a zero gradient and its rms decays. Which entries are touched is a matter of geometry and is taken
from the restatement (tests/grid_background_train_oracle.py); the gradients are autograd's.
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden_grid_background as MB  # noqa: E402  (this project's; imports svox2 from NERF_REFERENCE_SVOX2)
import make_golden_grid as MG  # noqa: E402

import grid_background_oracle as BO  # noqa: E402
import grid_background_train_oracle as BT  # noqa: E402
import grid_oracle as GO  # noqa: E402

svox2, ref_utils = MB.svox2, MB.ref_utils
F = np.float32
RESO, BASIS_DIM, RADIUS, CENTER, BG_RESO, NLAYERS, N_RAYS = MB.RESO, MB.BASIS_DIM, MB.RADIUS, MB.CENTER, MB.BG_RESO, MB.NLAYERS, MB.N_RAYS
# (nlayers, step_size, stop_thresh, background_brightness)
SETTINGS = [(2, 0.5, 1e-7, 1.0), (2, 0.3, 0.05, 0.0), (5, 0.5, 1e-7, 0.0), (5, 0.5, 0.05, 1.0), (5, 0.3, 1e-7, 1.0), (5, 0.3, 0.05, 0.0),
            (8, 0.5, 1e-7, 0.0), (8, 0.3, 0.05, 1.0)]
DENSE = 40000.0
LOOP_SETTING, N_ITERS, N_BATCH = 4, 20, 256
BETA, EPS, LR_SH, LR_SIGMA, LR_SIGMA_BG, LR_COLOR_BG = 0.95, 1e-8, 1e-2, 1.0, 0.5, 1e-2
SH_C0 = BO.SH_C0


class TakeTransmittance:
    """Stands where the reference's renderer reads ``opt.background_brightness``: ``exp(log_T).unsqueeze(-1) * self`` hands the
    transmittance over and adds nothing to the colour."""

    def __init__(self):
        self.value = None

    def __bool__(self):
        return True

    def __rmul__(self, t):
        self.value = t[:, 0]
        return torch.zeros_like(t)


def make_foreground(rng):
    links, density, sh = MG.make_grid(rng, "bgt", RESO, BASIS_DIM)
    n = density.shape[0]
    density = (np.round(rng.uniform(-0.3, 1.0, (n, 1)) * 16) / 16).astype(F)      # light: no ray reaches 0.05 through it
    dense = rng.choice(n, 8, replace=False)
    density[dense] = DENSE
    return links, density, sh, dense


def make_rays(rng, grid, dense_rows):
    o, d = MB.make_rays(rng)
    radius, center = np.array(RADIUS), np.array(CENTER)
    # 288..319: towards the -y pole (l_y = R - 1: the y seam), from inside the unit sphere
    k = np.arange(288, 320)
    d[k] = np.stack([rng.uniform(-0.25, 0.25, len(k)), -np.ones(len(k)), rng.uniform(-0.25, 0.25, len(k))], -1) * radius
    # 320..351: from outside, aimed at one of the very dense nodes
    k = np.arange(320, 352)
    pos = np.argwhere(np.isin(grid["links"], dense_rows))
    target = pos[rng.integers(0, len(pos), len(k))] + rng.uniform(-0.2, 0.2, (len(k), 3))
    world = center + radius * ((target + 0.5) / np.array(RESO) * 2.0 - 1.0)
    u = rng.normal(size=(len(k), 3))
    o[k] = center + 2.5 * radius * u / np.linalg.norm(u, axis=-1, keepdims=True)
    d[k] = world - o[k]
    return o.astype(F), d.astype(F)


def borderline(grid, o, d):
    """rays whose fp32 foreground log_T after some sample lies in [-25, log(0.05) + 0.05], at either step size, or whose
    inner radius is within 1e-4 of a sphere's"""
    bad = np.zeros(o.shape[0], bool)
    lo, hi = -25.0, np.log(0.05) + 0.05

    def shade(rays, lk, wa, wb, sigma, raw, weight, log_t):
        bad[rays[(log_t >= lo) & (log_t <= hi)]] = True

    for step in (0.5, 0.3):
        GO.march_colour(grid, o, d, step, 0.0, 0.0, shade=shade)
    og, dg, _, ds, _, _, ok = GO.ray_setup(grid, o, d)
    su = BO.setup(np.where(ok[:, None], og, 0), np.where(ok[:, None], dg, 1), np.where(ok, ds, 1), RESO, np.float64)
    all_radii = np.unique(np.concatenate([BO.radii(nl, st) for nl, st, _, _ in SETTINGS]))
    bad |= ok & (np.abs(su["inner"][:, None] - all_radii[None, :].astype(np.float64)) < 1e-4).any(-1)
    return bad


def ref_foreground(grid, o, d, step_size, dtype):
    """(reference grid with grad-enabled tables, rgb [n, 3], exp(log_T) [n]) of the finite rays, by the reference's renderer"""
    g = MG.ref_grid(RESO, RADIUS, CENTER, BASIS_DIM, grid["links"], grid["density_data"], grid["sh_data"], dtype)
    g.density_data.requires_grad_(True)
    g.sh_data.requires_grad_(True)
    take = TakeTransmittance()
    g.opt.background_brightness, g.opt.step_size, g.opt.near_clip = take, step_size, 0.0
    rays = svox2.Rays(torch.from_numpy(o).to(dtype), torch.from_numpy(d).to(dtype))
    rgb = g._volume_render_gradcheck_lerp(rays)
    return g, rgb, take.value


def background_torch(setup, bg_links, bg_data, log_t, nlayers, step_size, stop_thresh, brightness, dtype):
    """The header's forward on rays with a finite set-up that are not left alone: (colour added [n, 3], final log_T [n])."""
    og, dg, ds = setup
    t = lambda a: torch.from_numpy(np.asarray(a, F)).to(dtype)      # noqa: E731
    csi = ref_utils.ConcentricSpheresIntersector(t(np.array(RESO, F)), t(og), t(dg), t(ds))
    inner = (torch.cross(csi.origins, csi.dirs, dim=-1).norm(dim=-1) + 1e-3).clamp_min(1.0)
    invr_last = 1.0 / inner
    R, L = BG_RESO, nlayers
    links = torch.from_numpy(bg_links.astype(np.int64)).reshape(-1)
    n = log_t.shape[0]
    out = torch.zeros((n, 3), dtype=dtype)
    live = torch.ones(n, dtype=torch.bool)
    lerp = lambda a, b, w: a + w * (b - a)      # noqa: E731
    for r in BO.radii(L, step_size):
        r = float(r)
        hit, tt = csi.intersect(r)
        taken = hit & ~(r < inner)
        pos = csi.origins + tt.unsqueeze(-1) * csi.dirs
        invr = 1.0 / pos.norm(dim=-1)
        xy = ref_utils.xyz2equirect(pos * invr.unsqueeze(-1), R)
        z = torch.clamp((1.0 - invr) * L - 0.5, 0.0, L - 1)
        lx = xy[:, 0].to(torch.long).clamp(0, 2 * R - 1)
        ly = xy[:, 1].to(torch.long).clamp(0, R - 1)
        lz = z.to(torch.long).clamp(0, L - 2)
        wx, wy, wz = (xy[:, 0] - lx).unsqueeze(-1), (xy[:, 1] - ly).unsqueeze(-1), (z - lz).unsqueeze(-1)
        nx, ny = (lx + 1) % (2 * R), (ly + 1) % R

        def texel(X, Y):
            lk = links[X * R + Y]
            has = (lk >= 0).unsqueeze(-1)
            row = lk.clamp_min(0)
            return torch.where(has, lerp(bg_data[row, lz], bg_data[row, lz + 1], wz), torch.zeros((), dtype=dtype))

        v = lerp(lerp(texel(lx, ly), texel(lx, ny), wy), lerp(texel(nx, ly), texel(nx, ny), wy), wx)
        cur = live & taken
        sh = cur & (v[:, 3] > 0)
        p = ((invr_last - invr) * csi.world_step_scale) * v[:, 3]
        weight = torch.exp(log_t) * (1.0 - torch.exp(-p))
        col = torch.clamp_min(v[:, :3] * SH_C0 + 0.5, 0.0)
        out = out + torch.where(sh.unsqueeze(-1), weight.unsqueeze(-1) * col, torch.zeros((), dtype=dtype))
        log_t = torch.where(sh, log_t - p, log_t)
        stop = sh & (torch.exp(log_t.detach()) < stop_thresh)
        invr_last = torch.where(cur & ~stop, invr, invr_last)
        live = live & ~stop
    return out + (torch.exp(log_t) * brightness).unsqueeze(-1), log_t


def composite(grid, bg, o, d, setup, ok, setting, dtype):
    """(reference grid, background_data leaf, rgb [n, 3] of all rays, foreground log_T [n] as numpy) in ``dtype``"""
    nl, step, stop, bright = setting
    n = o.shape[0]
    fin = np.nonzero(ok)[0]
    torch.set_default_dtype(dtype)
    try:
        g, fg_rgb, T = ref_foreground(grid, o[fin], d[fin], step, dtype)
        bg_data = torch.from_numpy(bg["data"]).to(dtype).requires_grad_(True)
        act = T.detach() >= float(np.exp(-25.0))      # the others are left alone
        ia = torch.nonzero(act)[:, 0]
        log_t = torch.log(T[ia])
        sub = tuple(a[fin][ia.numpy()] for a in setup)
        add, _ = background_torch(sub, bg["links"], bg_data, log_t, nl, step, stop, bright, dtype)
        rgb_fin = fg_rgb.index_add(0, ia, add)
        rgb = torch.full((n, 3), float(bright), dtype=dtype).index_copy(0, torch.from_numpy(fin), rgb_fin)
        logt = np.zeros(n)
        with np.errstate(divide="ignore"):
            logt[fin] = np.log(T.detach().numpy().astype(np.float64))
    finally:
        torch.set_default_dtype(torch.float32)
    return g, bg_data, rgb, logt


def loss_and_grads(grid, bg, o, d, gt, setup, ok, setting, dtype):
    g, bg_data, rgb, logt = composite(grid, bg, o, d, setup, ok, setting, dtype)
    loss = ((rgb - torch.from_numpy(gt).to(dtype)) ** 2).mean()
    loss.backward()
    zero = lambda p: torch.zeros_like(p) if p.grad is None else p.grad      # noqa: E731
    return (loss.item(), zero(g.density_data).numpy().copy(), zero(g.sh_data).numpy().copy(), zero(bg_data).numpy().copy(),
            rgb.detach().numpy().copy(), logt)


def rmsprop(data, rms, grad, mask, lr):
    """the statement of include/nerf_mi355x.h in the arrays' own precision, on the masked entries"""
    dt = data.dtype.type
    g = grad[mask]
    g2 = g * g
    r = rms[mask]
    r = np.where(r == 0, g2, g2 + dt(BETA) * (r - g2))
    rms[mask] = r
    data[mask] = np.maximum(data[mask] - (dt(lr) * g) / (np.sqrt(r) + dt(EPS)), dt(-1e9))


def main():
    rng = np.random.default_rng(20250611)
    links, density, sh, dense = make_foreground(rng)
    grid = {"links": links, "density_data": density, "sh_data": sh, "radius": np.array(RADIUS, F), "center": np.array(CENTER, F)}
    o, d = make_rays(rng, grid, dense)
    for attempt in range(200):
        bad = borderline(grid, o, d)
        if not bad.any():
            break
        o2, d2 = make_rays(rng, grid, dense)
        o[bad], d[bad] = o2[bad], d2[bad]
    assert not bad.any()
    og, dg, _, ds, _, _, ok = GO.ray_setup(grid, o, d)
    setup = (og, dg, ds)
    gt = rng.uniform(0.0, 1.0, (N_RAYS, 3)).astype(F)
    out = {"links": links, "density": density, "sh": sh, "radius": np.array(RADIUS, F), "center": np.array(CENTER, F),
           "origins": o, "dirs": d, "rgb_gt": gt, "setup_ok": ok, "settings": np.array(SETTINGS, dtype=np.float64)}
    bgs = {}
    for nl in NLAYERS:
        bl, bd = MB.make_background(rng, nl)
        bgs[nl] = {"links": bl, "data": bd}
        out[f"bg{nl}_links"], out[f"bg{nl}_data"] = bl, bd
    cover = dict(left_alone=0, stopped=0, seam_x=0, seam_y=0, clamped=0)
    for j, setting in enumerate(SETTINGS):
        nl, step, stop, bright = setting
        bg = bgs[nl]
        r32 = loss_and_grads(grid, bg, o, d, gt, setup, ok, setting, torch.float32)
        r64 = loss_and_grads(grid, bg, o, d, gt, setup, ok, setting, torch.float64)
        out[f"set{j}_loss64"] = np.float64(r64[0])
        out[f"set{j}_rgb64"], out[f"set{j}_fg_logt64"] = r64[4], r64[5]
        out[f"set{j}_grad_density64"] = r64[1].astype(F)      # (rounded to fp32 for the size of the file: a relative 6e-8)
        out[f"set{j}_grad_sh64"] = r64[2].astype(F)
        out[f"set{j}_grad_background64"] = r64[3]              # (kept in fp64: the fp64 restatement is compared to 1e-10)
        for key, a32, a64 in (("density", r32[1], r64[1]), ("sh", r32[2], r64[2]), ("background", r32[3], r64[3])):
            assert a32.dtype == np.float32 and a64.dtype == np.float64
            d_ref = float(np.abs(a32.astype(np.float64) - a64).max())
            out[f"set{j}_grad_{key}_d_ref"] = np.float64(d_ref)
            print(f"setting {j} {setting} d/d{key}: max |g64| {np.abs(a64).max():.3e}, |fp32 - fp64| max {d_ref:.3e}, "
                  f"rows != 0: {int((a64.reshape(a64.shape[0], -1) != 0).any(-1).sum())} of {a64.shape[0]}")
        # the restatement's view of the same setting: the kernels' stop rule in the foreground, and the coverage
        res = BT.forward_backward(grid, bg, o, d, gt, step, 0.0, stop, bright)
        fg_rgb, fg_logt, (_, _, _, tot), _ = GO.march_colour(grid, o, d, step, 0.0, stop)
        st = BT.taped(og, dg, ds, ok, RESO, bg, fg_rgb, fg_logt, tot, step, stop, bright, return_stats=True)[4]
        st64 = BT.taped(og, dg, ds, ok, RESO, bg, fg_rgb, fg_logt, tot, step, stop, bright, T=np.float64, return_stats=True)[4]
        assert (st["shaded"] == st64["shaded"]).all() and (st["stopped"] == st64["stopped"]).all(), "a ray stops in one precision only"
        assert ((fg_logt < -25) == (r64[5] < -25)).all(), "left alone in one statement only"
        err = float(np.abs(res["rgb"].astype(np.float64) - r64[4]).max())
        rgb_d_ref = float(np.abs(r32[4].astype(np.float64) - r64[4]).max())
        out[f"set{j}_rgb_d_ref"] = np.float64(rgb_d_ref)
        assert err <= max(3.0 * rgb_d_ref, 1e-5), (err, rgb_d_ref)      # the two statements of the forward agree
        rows = int((r64[3].reshape(r64[3].shape[0], -1) != 0).any(-1).sum())
        assert 2 * rows >= r64[3].shape[0], (rows, r64[3].shape[0])
        cover["left_alone"] = max(cover["left_alone"], int((st["left_alone"] & ok).sum()))
        if stop == 0.05:
            cover["stopped"] = max(cover["stopped"], int(st["stopped"].sum()))
        for key in ("seam_x", "seam_y", "clamped"):
            cover[key] = max(cover[key], int(st[key].sum()))
        print(f"setting {j}: restated rgb vs fp64 autograd {err:.2e}; left alone {int((st['left_alone'] & ok).sum())}, stopped "
              f"{int(st['stopped'].sum())}, seam x {int(st['seam_x'].sum())}, seam y {int(st['seam_y'].sum())}, clamped "
              f"{int(st['clamped'].sum())}, background rows with a gradient {rows} of {r64[3].shape[0]}")
    print(cover)
    assert min(cover.values()) >= 16, cover
    # ---- a 20-iteration RMSProp loop on all three tables ----
    setting = SETTINGS[LOOP_SETTING]
    nl = int(setting[0])
    pool = np.nonzero(ok)[0]
    idx = np.stack([rng.choice(pool, N_BATCH, replace=False) for _ in range(N_ITERS)]).astype(np.int32)
    target = out[f"set{LOOP_SETTING}_rgb64"]
    out["loop_idx"], out["loop_params"] = idx, np.array([BETA, EPS, LR_SH, LR_SIGMA, LR_SIGMA_BG, LR_COLOR_BG])
    res = {}
    for dtype, tag in ((torch.float32, "32"), (torch.float64, "64")):
        npdt = np.float32 if dtype == torch.float32 else np.float64
        g = dict(grid, density_data=(0.5 * np.minimum(density, 2.0)).astype(F).astype(npdt), sh_data=np.zeros_like(sh).astype(npdt))
        b = dict(links=bgs[nl]["links"], data=(0.5 * bgs[nl]["data"]).astype(F).astype(npdt))
        rms = [np.zeros_like(g["density_data"]), np.zeros_like(g["sh_data"]), np.zeros_like(b["data"])]
        losses = []
        for it in range(N_ITERS):
            k = idx[it]
            loss, gd, gs, gb, _, _ = loss_and_grads(g, b, o[k], d[k], target[k].astype(npdt), tuple(a[k] for a in setup), ok[k], setting,
                                                    dtype)
            # the touched rows and (row, layer) entries, whatever their gradient (svox2's masks): a matter of the rays'
            # geometry, taken from the restatement on the current tables
            touched = BT.forward_backward(dict(g, density_data=g["density_data"].astype(F), sh_data=g["sh_data"].astype(F)),
                                          dict(b, data=b["data"].astype(F)), o[k], d[k], target[k].astype(F), setting[1], 0.0,
                                          setting[2], setting[3])
            mask = touched["mask"] != 0
            rmsprop(g["density_data"], rms[0], gd, mask, LR_SIGMA)
            rmsprop(g["sh_data"], rms[1], gs, mask, LR_SH)
            mb = touched["mask_background"] != 0
            lr = np.array([LR_COLOR_BG] * 3 + [LR_SIGMA_BG], dtype=npdt)
            for c in range(4):
                dc, rc = b["data"][..., c], rms[2][..., c]
                rmsprop(dc, rc, gb[..., c], mb, lr[c])
            losses.append(loss)
        res[tag] = (np.array(losses, np.float64), g["density_data"].copy(), g["sh_data"].copy(), b["data"].copy())
    for i, key in enumerate(("loss", "density", "sh", "background")):
        out[f"loop_{key}32"], out[f"loop_{key}64"] = res["32"][i], res["64"][i]
    l32, l64 = res["32"][0], res["64"][0]
    print(f"loop: loss {l64[0]:.5f} -> {l64[-1]:.5f}, max |l32 - l64| {np.abs(l32 - l64).max():.2e}; final |32 - 64| density "
          f"{np.abs(res['32'][1] - res['64'][1]).max():.2e}, sh {np.abs(res['32'][2] - res['64'][2]).max():.2e}, background "
          f"{np.abs(res['32'][3] - res['64'][3]).max():.2e}")
    assert np.abs(l32 - l64).max() < 1e-3 * (l64[0] - l64[-1])      # the fixture must test the optimisation, not noise
    path = os.path.join(HERE, "grid_background_train.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        main()
