"""Per-tensor gradient errors of the no-viewdirs training fixture (tests/golden/train_step_noviewdirs.npz): largest element error /
tensor's largest entry, and norm error. Run with and without the NERF_TRAIN_* switches. tools/gpu: run on the box."""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import nerf_projects_amd as N
from nerf_projects_amd import synthetic
g = np.load(ROOT + "/tests/golden/train_step_noviewdirs.npz")
arch = dict(input_ch_views=0, use_viewdirs=False, output_ch=5)
sd_c, sd_f = synthetic.synthetic_state_dict(8, **arch), synthetic.synthetic_state_dict(48, **arch)
mk = dict(D=8, W=256, input_ch=63, skips=[4], **arch)
net_c, net_f = N.NeRF(**mk).load_state_dict(sd_c), N.NeRF(**mk).load_state_dict(sd_f)
rays = torch.from_numpy(g["rays"]).cuda()
kw = dict(network_fn=net_c, network_fine=net_f, N_samples=64, N_importance=128, white_bkgd=True, perturb=1.0, raw_noise_std=1.0,
          pytest=True, ndc=False, use_viewdirs=False, near=2., far=6.)
opt = N.Adam([net_c, net_f], lr=5e-4)
ctx = N.get_context(); ctx.precision_detail(reset=True)
out = N.train_on_batch(800, 800, None, (rays[:, 0:3], rays[:, 3:6]), torch.from_numpy(g["target"]).cuda(), opt, apply_update=False, **kw)
print("env", {k: v for k, v in os.environ.items() if k.startswith("NERF_TRAIN_")}, "losses", float(out["img_loss"]) - float(g["img_loss"]), float(out["img_loss0"]) - float(g["img_loss0"]),
      "events", ctx.precision_detail())
for tag, net in (("c", net_c), ("f", net_f)):
    for k, gr in net.grad_dict().items():
        gr = gr.numpy().reshape(-1)
        want = g[f"gsub_{tag}.{k}"]
        top = np.abs(want).max() + 1e-30
        wn = float(g[f"gnorm_{tag}.{k}"])
        print(f"  {tag}.{k:26s} elem {np.abs(gr[::61] - want).max() / top:.2e}  norm {abs(np.linalg.norm(gr.astype(np.float64)) - wn) / (wn + 1e-30):.2e}")
