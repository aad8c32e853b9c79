#!/usr/bin/env python3
"""Writes tests/golden/train_occupancy.npz: the reference's training loop body (nerf.ipynb:1258-1282) with its network query
replaced by a MASKED query - the statement of ``train_on_batch(..., occupancy=occ)`` (include/nerf_mi355x.h, "Occupancy
grid"). Runs on the CPU; reads the reference through make_golden.py. Nothing of the reference is copied: arrays only.

    python tests/golden/make_golden_train_occupancy.py

The wrapper around ``network_query_fn``:
  * computes the keep mask of the ``[N, S, 3]`` points from a hand-made cell mask (``np_keep`` of tests/test_occupancy_cpu.py,
    on the points rounded to fp32), the last sample of every ray forced to kept;
  * multiplies the network's output by the mask;
  * with noise on, adds the sigma noise to the KEPT samples only - the draws of ``raw2outputs``' pytest mode, which are those of
    ``train_on_batch(pytest=True)`` - and ``raw2outputs`` itself gets ``raw_noise_std = 0``.
Every case runs in fp32 and in fp64 (the fp64 run resamples at the fp32 run's z_samples, so that both differentiate the same
samples). Stored: both losses of both runs, rgb, rgb0 and the fine depths of the fp32 run, per gradient tensor its norm in both
precisions and every 61st entry of the fp32 run with its largest distance from the fp64 run's, every 487th entry of the
weights after the Adam step with the rms distance between the runs (and the count of entries more than 0.2 lr apart) - the
fp64 arrays themselves would double the file for two numbers per tensor. Also the reference's PLAIN loop body on the same
inputs (``unmasked.*``), which mask (iv) must reproduce.

Shape: the 8 x 256 networks of ``synthetic.synthetic_pair(0)``, 48 rays of the bench frame, 16 + 32 samples, perturb = 1 with
the pytest RNG, white background. Grid: [-1.5, 1.5]^3, 17 nodes per axis. Masks: (i) ``ball`` - the cells whose centre lies
within a radius of the origin; (ii) ``checker`` - a 3-D checkerboard of single cells; (iii) ``empty``; (iv) ``full``. (i) and
(ii) run with both ``outside`` modes. A sample within 1e-4 of a cell face (in cell units) could be classified differently by
fp32 on the device: rays holding one at the coarse or the recorded fine depths of ANY case are drawn again until none is left
(asserted; the count is printed).

The loop: 20 iterations under ``ball`` / outside = "empty" at N_rand = 64 from freshly initialised networks, losses in fp32
and fp64, like train_loop.npz. Its fine depths move with the weights, so rays cannot be redrawn one by one: the batch seed is
the first for which no sample of the fp32 run comes within 5e-6 of a face (a few ulps of the cell coordinate).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  (this project's; imports the reference)
from test_occupancy_cpu import np_keep  # noqa: E402

F32 = np.float32
C1, C2, RESO = -1.5, 1.5, 17
NC = RESO - 1
N_RAYS, SC, SI = 48, 16, 32
FACE_EPS = 1e-4
BALL_RADIUS = 1.3      # kept fraction of (i) with outside = "empty": 0.3 - 0.5 (asserted below)
W_STRIDE = 487         # the weights after the Adam step: every 487th entry (the gradients: every 61st)


def masks():
    c = (np.arange(NC) + 0.5) * ((C2 - C1) / NC) + C1
    X, Y, Z = np.meshgrid(c, c, c, indexing="ij")
    ball = (X ** 2 + Y ** 2 + Z ** 2) <= BALL_RADIUS ** 2
    i, j, k = np.meshgrid(np.arange(NC), np.arange(NC), np.arange(NC), indexing="ij")
    checker = ((i + j + k) % 2) == 0
    return {"ball": ball, "checker": checker, "empty": np.zeros((NC,) * 3, bool), "full": np.ones((NC,) * 3, bool)}


CASES = (("ball_eval", "ball", "evaluate", 0.0), ("ball_empty", "ball", "empty", 0.0),
         ("checker_eval", "checker", "evaluate", 0.0), ("checker_empty", "checker", "empty", 0.0),
         ("empty", "empty", "empty", 0.0), ("full", "full", "evaluate", 0.0), ("ball_empty_noise", "ball", "empty", 1.0))


def near_face(pts):
    """[N, S] True where a point lies within FACE_EPS (cell units) of a cell face or of the box's faces, on any axis."""
    t = (np.asarray(pts, np.float64) - C1) / ((C2 - C1) / NC)
    d = np.abs(t - np.round(t))
    return ((d < FACE_EPS) & (t > -1.0) & (t < NC + 1.0)).any(-1)


def masked_query(cells, outside, noise_std, rec):
    e_fn, _ = MG.ref_embedder.get_embedder(10, 0)
    ed_fn, _ = MG.ref_embedder.get_embedder(4, 0)
    plain = MG.query_fn(e_fn, ed_fn)

    def query(inputs, viewdirs, network_fn):
        pts = MG.n(inputs).astype(F32)
        keep = np_keep(pts, cells, C1, C2, outside)
        keep[..., -1] = True
        rec["pts"].append(pts)
        rec["keep"].append(keep)
        m = torch.from_numpy(keep).to(inputs.dtype)
        raw = plain(inputs, viewdirs, network_fn) * m[..., None]
        if noise_std > 0.0:
            np.random.seed(0)      # (raw2outputs' pytest draw, nerf.ipynb:312-325)
            noise = torch.from_numpy(np.random.rand(*keep.shape) * noise_std).to(inputs.dtype)
            raw = torch.cat([raw[..., :3], raw[..., 3:] + (noise * m)[..., None]], -1)
        return raw
    return query


def run_step(rays_np, target_np, sd_c, sd_f, cells, outside, noise_std, dtype, z_samples=None, lr=5e-4):
    """One iteration of the loop body; z_samples: resample at these instead of sample_pdf's (the fp64 run)."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    rec = {"pts": [], "keep": [], "z_samples": None, "z_vals": []}
    orig_pdf, orig_r2o = MG.NS["sample_pdf"], MG.NS["raw2outputs"]

    def r2o(raw, z_vals, rays_d, *a, **k):
        rec["z_vals"].append(MG.n(z_vals))
        return orig_r2o(raw, z_vals, rays_d, *a, **k)

    def pdf(bins, weights, N_samples, **k):
        out = orig_pdf(bins, weights, N_samples, **k)
        if z_samples is not None:
            out = torch.from_numpy(z_samples).to(out.dtype)
        rec["z_samples"] = MG.n(out)
        return out

    MG.NS["sample_pdf"], MG.NS["raw2outputs"] = pdf, r2o
    try:
        net_c, net_f = MG.ref_model(None, dtype, sd=sd_c), MG.ref_model(None, dtype, sd=sd_f)
        net_c.train(); net_f.train()
        opt = torch.optim.Adam(params=list(net_c.parameters()) + list(net_f.parameters()), lr=lr, betas=(0.9, 0.999))
        rays, target = torch.from_numpy(rays_np).to(dtype), torch.from_numpy(target_np).to(dtype)
        ret = MG.NS["render_rays"](rays, net_c, masked_query(cells, outside, noise_std, rec), network_fine=net_f,
                                   N_samples=SC, N_importance=SI, retraw=True, white_bkgd=True, perturb=1.0,
                                   raw_noise_std=0.0, pytest=True)
        opt.zero_grad()
        img_loss, img_loss0 = MG.ref_helpers.img2mse(ret["rgb_map"], target), MG.ref_helpers.img2mse(ret["rgb0"], target)
        (img_loss + img_loss0).backward()
        out = {"img_loss": img_loss.item(), "img_loss0": img_loss0.item(), "rgb": MG.n(ret["rgb_map"]), "rgb0": MG.n(ret["rgb0"])}
        for tag, net in (("c", net_c), ("f", net_f)):
            for k, p in net.named_parameters():
                gr = MG.n(p.grad).reshape(-1) if p.grad is not None else np.zeros(p.numel())
                out[f"gnorm_{tag}.{k}"] = np.linalg.norm(gr.astype(np.float64))
                out[f"gsub_{tag}.{k}"] = gr[::61].copy()
        opt.step()
        for tag, net in (("c", net_c), ("f", net_f)):
            for k, p in net.named_parameters():
                out[f"wsub_{tag}.{k}"] = MG.n(p).reshape(-1)[::W_STRIDE].copy()
    finally:
        MG.NS["sample_pdf"], MG.NS["raw2outputs"] = orig_pdf, orig_r2o
        torch.set_default_dtype(old)
    return out, rec


def gold_steps(out):
    frame = np.load(os.path.join(HERE, "bench_frame.npz"))
    rs = np.random.RandomState(311)
    pool = list(rs.permutation(len(frame["rays"])))
    sel = [pool.pop() for _ in range(N_RAYS)]
    target = rs.uniform(0, 1, size=(N_RAYS, 3)).astype(F32)
    sd_c, sd_f = MG.synthetic.synthetic_pair(0)
    M = masks()
    redrawn = 0
    while True:
        rays = frame["rays"][sel].astype(F32)
        bad = np.zeros(N_RAYS, bool)
        runs = {}
        for name, mask, outside, noise in CASES:
            res, rec = run_step(rays, target, sd_c, sd_f, M[mask], outside, noise, torch.float32)
            runs[name] = (res, rec)
            for pts in rec["pts"]:
                bad |= near_face(pts).any(-1)
        if not bad.any():
            break
        for i in np.nonzero(bad)[0]:
            sel[i] = pool.pop()
            redrawn += 1
    print(f"  rays redrawn because a sample lay within {FACE_EPS} of a cell face: {redrawn}")
    for name, (res, rec) in runs.items():
        for pts in rec["pts"]:
            assert not near_face(pts).any()
    out.update(rays=rays, target=target, sel=np.array(sel), c1=C1, c2=C2, reso=RESO, n_samples=SC, n_importance=SI,
               face_eps=FACE_EPS, redrawn=redrawn, **MG.pair_digests(0))
    for k, m in M.items():
        out[f"mask.{k}"] = np.packbits(m.reshape(-1))
    for name, mask, outside, noise in CASES:
        res, rec = runs[name]
        res64, rec64 = run_step(rays, target, sd_c, sd_f, M[mask], outside, noise, torch.float64, z_samples=rec["z_samples"])
        assert all(np.array_equal(a, b) for a, b in zip(rec["keep"], rec64["keep"])), name      # both runs keep the same samples
        out[f"{name}.mask"], out[f"{name}.outside"], out[f"{name}.noise_std"] = mask, outside, noise
        out[f"{name}.z_fine"] = rec["z_vals"][1].astype(F32)      # the fine pass's depths of the fp32 run
        out[f"{name}.kept_c"], out[f"{name}.kept_f"] = int(rec["keep"][0].sum()), int(rec["keep"][1].sum())
        out[f"{name}.kept_fraction"] = (rec["keep"][0].sum() + rec["keep"][1].sum()) / float(N_RAYS * (SC + SC + SI))
        out[f"{name}.keep_c"] = np.packbits(rec["keep"][0].reshape(-1))
        out[f"{name}.keep_f"] = np.packbits(rec["keep"][1].reshape(-1))
        # One array per kind and network (a zip entry per tensor would cost more than its data): the parameters in
        # named_parameters() order (`names_c` / `names_f`), the sampled entries concatenated (`gsub_len_*`, `wsub_len_*`: entries
        # per tensor). Of the fp64 run: the scalars, the norms, and only the DISTANCE of its sampled arrays from the fp32 run
        # (the yardstick) - per tensor the largest entry for the gradients, rms and entries > 0.2 lr apart for the weights.
        for k in ("img_loss", "img_loss0"):
            out[f"{name}.{k}"], out[f"{name}.{k}.f64"] = res[k], res64[k]
        out[f"{name}.rgb"], out[f"{name}.rgb0"] = res["rgb"].astype(F32), res["rgb0"].astype(F32)
        for tag in ("c", "f"):
            names = [k[len(f"gsub_{tag}."):] for k in res if k.startswith(f"gsub_{tag}.")]
            out[f"names_{tag}"] = np.array(names)
            out[f"gsub_len_{tag}"] = np.array([len(res[f"gsub_{tag}.{k}"]) for k in names])
            out[f"wsub_len_{tag}"] = np.array([len(res[f"wsub_{tag}.{k}"]) for k in names])
            out[f"{name}.gnorm_{tag}"] = np.array([res[f"gnorm_{tag}.{k}"] for k in names])
            out[f"{name}.gnorm_{tag}.f64"] = np.array([res64[f"gnorm_{tag}.{k}"] for k in names])
            out[f"{name}.ggap_{tag}"] = np.array([np.abs(res[f"gsub_{tag}.{k}"].astype(np.float64) - res64[f"gsub_{tag}.{k}"]).max()
                                                   for k in names])
            if mask != "full":      # (iv) is compared with the dense step on the device, not with this file
                out[f"{name}.gsub_{tag}"] = np.concatenate([res[f"gsub_{tag}.{k}"] for k in names]).astype(F32)
                out[f"{name}.wsub_{tag}"] = np.concatenate([res[f"wsub_{tag}.{k}"] for k in names]).astype(F32)
            d = np.concatenate([res[f"wsub_{tag}.{k}"].astype(np.float64) - res64[f"wsub_{tag}.{k}"] for k in names])
            out[f"{name}.wgap_rms_{tag}"], out[f"{name}.wgap_far_{tag}"] = float(np.sqrt(np.mean(d ** 2))), int((np.abs(d) > 0.2 * 5e-4).sum())
        print(f"  {name}: kept {out[f'{name}.kept_c']} + {out[f'{name}.kept_f']} ({out[f'{name}.kept_fraction']:.3f}), losses "
              f"{res['img_loss']:.6f} {res['img_loss0']:.6f} (fp64 {res64['img_loss']:.6f} {res64['img_loss0']:.6f})")


def run_loop(rays_np, target_np, idx, cells, dtype, n_iters, lr=5e-4):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        sd_c, sd_f = MG.synthetic.default_init_state_dict(11), MG.synthetic.default_init_state_dict(12)
        net_c, net_f = MG.ref_model(None, dtype, sd=sd_c), MG.ref_model(None, dtype, sd=sd_f)
        net_c.train(); net_f.train()
        opt = torch.optim.Adam(params=list(net_c.parameters()) + list(net_f.parameters()), lr=lr, betas=(0.9, 0.999))
        losses, losses0, closest = [], [], 1.0
        for it in range(n_iters):
            rec = {"pts": [], "keep": []}
            rays, target = torch.from_numpy(rays_np[idx[it]]).to(dtype), torch.from_numpy(target_np[idx[it]]).to(dtype)
            ret = MG.NS["render_rays"](rays, net_c, masked_query(cells, "empty", 1.0, rec), network_fine=net_f, N_samples=SC,
                                       N_importance=SI, retraw=True, white_bkgd=True, perturb=1.0, raw_noise_std=0.0, pytest=True)
            opt.zero_grad()
            img_loss, img_loss0 = MG.ref_helpers.img2mse(ret["rgb_map"], target), MG.ref_helpers.img2mse(ret["rgb0"], target)
            (img_loss + img_loss0).backward()
            opt.step()
            losses.append(img_loss.item()); losses0.append(img_loss0.item())
            for pts in rec["pts"]:
                t = (pts.astype(np.float64) - C1) / ((C2 - C1) / NC)
                d = np.abs(t - np.round(t))[(t > -1.0) & (t < NC + 1.0)]
                closest = min(closest, float(d.min()))
        wsub = {f"wsub_{tag}.{k}": MG.n(p).reshape(-1)[::W_STRIDE].copy() for tag, net in (("c", net_c), ("f", net_f))
                for k, p in net.named_parameters()}
    finally:
        torch.set_default_dtype(old)
    return np.array(losses), np.array(losses0), closest, wsub


def gold_unmasked(out):
    """The reference's plain loop body on the step fixture's inputs (no wrapper, raw2outputs draws no noise): what mask (iv)
    must reproduce."""
    sd_c, sd_f = MG.synthetic.synthetic_pair(0)
    e_fn, _ = MG.ref_embedder.get_embedder(10, 0)
    ed_fn, _ = MG.ref_embedder.get_embedder(4, 0)
    net_c, net_f = MG.ref_model(None, torch.float32, sd=sd_c), MG.ref_model(None, torch.float32, sd=sd_f)
    net_c.train(); net_f.train()
    rays, target = torch.from_numpy(out["rays"]), torch.from_numpy(out["target"])
    ret = MG.NS["render_rays"](rays, net_c, MG.query_fn(e_fn, ed_fn), network_fine=net_f, N_samples=SC, N_importance=SI,
                               retraw=True, white_bkgd=True, perturb=1.0, raw_noise_std=0.0, pytest=True)
    img_loss, img_loss0 = MG.ref_helpers.img2mse(ret["rgb_map"], target), MG.ref_helpers.img2mse(ret["rgb0"], target)
    (img_loss + img_loss0).backward()
    out["unmasked.img_loss"], out["unmasked.img_loss0"] = img_loss.item(), img_loss0.item()
    out["unmasked.rgb"] = MG.n(ret["rgb_map"])
    for tag, net in (("c", net_c), ("f", net_f)):
        out[f"unmasked.gnorm_{tag}"] = np.array([np.linalg.norm(MG.n(p.grad).reshape(-1).astype(np.float64))
                                                 for _, p in net.named_parameters()])


def gold_loop(out, n_iters=20, n_rand=64):
    frame = np.load(os.path.join(HERE, "bench_frame.npz"))
    u, v = (frame["pix"] % 800) / 799.0, (frame["pix"] // 800) / 799.0
    ramp = np.stack([u, v, 1.0 - u], -1)
    target = np.clip(0.6 * frame["rgb_map"].astype(np.float64) + 0.4 * ramp, 0.0, 1.0).astype(F32)
    rays = frame["rays"].astype(F32)
    cells = masks()["ball"]
    for seed in range(400, 440):
        perm = np.random.RandomState(seed).permutation(len(rays))
        idx = [perm[(i * n_rand) % len(perm):(i * n_rand) % len(perm) + n_rand] for i in range(n_iters)]
        l32, l032, closest, w32 = run_loop(rays, target, idx, cells, torch.float32, n_iters)
        print(f"  loop seed {seed}: closest sample to a face {closest:.2e} cells")
        if closest >= 5e-6:
            break
    else:
        raise AssertionError("no batch seed keeps every sample of the loop 5e-6 cells off the faces")
    l64, l064, _, w64 = run_loop(rays, target, idx, cells, torch.float64, n_iters)
    out.update({"loop.seed": seed, "loop.perm": perm.astype(np.int16), "loop.target": target, "loop.n_rand": n_rand, "loop.n_iters": n_iters,
                "loop.lrate": 5e-4, "loop.closest_face": closest, "loop.img_loss": l32, "loop.img_loss0": l032,
                "loop.img_loss.f64": l64, "loop.img_loss0.f64": l064,
                "loop.digest_c": MG.synthetic.state_dict_digest(MG.synthetic.default_init_state_dict(11)),
                "loop.digest_f": MG.synthetic.state_dict_digest(MG.synthetic.default_init_state_dict(12))})
    for tag in ("c", "f"):
        out[f"loop.wsub_{tag}"] = np.concatenate([v for k, v in w32.items() if k.startswith(f"wsub_{tag}.")]).astype(F32)
        d = np.concatenate([w32[k].astype(np.float64) - w64[k] for k in w32 if k.startswith(f"wsub_{tag}.")])
        out[f"loop.wgap_rms_{tag}"], out[f"loop.wgap_far_{tag}"] = float(np.sqrt(np.mean(d ** 2))), int((np.abs(d) > 0.2 * 5e-4).sum())
    print("  loop losses fp32:", np.round(l32, 6)[[0, 1, n_iters - 1]], "fp64:", np.round(l64, 6)[[0, 1, n_iters - 1]],
          "largest gap", np.abs(l32 - l64).max(), np.abs(l032 - l064).max())


if __name__ == "__main__":
    out = {}
    gold_steps(out)
    gold_unmasked(out)
    gold_loop(out)
    assert 0.3 <= out["ball_empty.kept_fraction"] <= 0.5, out["ball_empty.kept_fraction"]
    assert out["empty.kept_c"] == N_RAYS and out["empty.kept_f"] == N_RAYS and out["full.kept_fraction"] == 1.0
    out["w_stride"] = W_STRIDE
    MG.save("train_occupancy", **out)
