"""A/B of the colour row's lane mapping (profiles/octree.md): one lane per ray against a lane group per ray, alternated step by
step in one process; wrote profiles/bench_octree_lanes_ab.json.

    git apply profiles/microbench/octree_group_lanes.patch && python nerf-projects_amd/build.py
    python profiles/microbench/octree_lanes_ab.py

The patch adds the group kernel and the switch NERF_OCTREE_LANES=group, read at every render call, to the three octree sources.
"""
import json, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
torch.cuda.set_device(0)
import nerf_projects_amd as N
from nerf_projects_amd import synthetic
arch = dict(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=4, skips=[4], use_viewdirs=True)
_, sd_f = synthetic.synthetic_pair(0)
net_f = N.NeRF(**arch).load_state_dict(sd_f)
H = W = 800
K, c2w, _, _ = synthetic.lego_camera(H, W)
cam = N.Camera.from_nerf_pose(c2w, H, W, float(K[0][0]))
def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); r = fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1), r
out = {}
for R in (128, 256):
    grid = N.SparseGrid.from_nerf(net_f, -1.5, 1.5, R, n_dirs=64)
    tree = N.N3Tree.from_grid(grid)
    times = {"lane": [], "group": []}
    imgs = {}
    for step in range(3 + 15):
        for leg in ("lane", "group"):
            os.environ["NERF_OCTREE_LANES"] = leg
            ms, img = timed(lambda: tree.volume_render_image(cam, step_size=1e-3))
            imgs[leg] = img
            if step >= 3:
                times[leg].append(ms)
    os.environ["NERF_OCTREE_LANES"] = "lane"
    diff = float((imgs["lane"] - imgs["group"]).abs().max())
    out[R] = {leg: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))} for leg, v in times.items()}
    out[R]["max_abs_diff"] = diff
    out[R]["nodes"] = tree.n_internal
    assert diff < 1e-4, diff
print(json.dumps(out))
