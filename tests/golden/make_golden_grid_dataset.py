"""Writes tests/golden/grid_dataset.npz: what the reference's svox2 training script gives for the training rays of
tests/golden/tiny_scene/blender (3 images of 16 x 16 RGBA) and for its learning-rate schedule.

    NERF_REFERENCE_SVOX2=/path/to/reference/svox2 python tests/golden/make_golden_grid_dataset.py

Runs on the CPU in seconds. The reference's ``opt/util/nerf_dataset.py`` is imported and run as it is; ``cv2`` and ``imageio``
are not installed, so stand-ins are put into ``sys.modules`` before the import: an ``imageio`` whose ``imread`` decodes with
Pillow (imageio's own PNG backend) and an empty ``cv2`` (the loader calls it only for ``scale < 1``). Nothing of the
reference is copied: the fixture holds arrays only.

(a) ``NeRFDataset(root, "train", factor=f)`` for f = 1, 2, 3 (16 // 3 = 5: windows that the factor does not divide): the
    fp32 ``rays_init`` (origins, dirs, gt), the poses after the OpenGL -> OpenCV flip and the scene scale, the fp64
    intrinsics, and the decoded uint8 images.
(b) the same formulas evaluated in fp64 by this script (pixel centres at + 0.5, normalise, rotate; u8 / 255 composited over
    white, averaged over torch's area windows), and ``d_dirs_f`` / ``d_gt_f`` = max |reference fp32 - fp64|: the reference's
    own distance from exact arithmetic, from which the tests take their bar.
(c) ``get_expon_lr_func`` at a list of steps for three parameter sets: opt.py's defaults for sigma (with a delay) and for SH,
    and a short schedule that reaches its end inside the list.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SCENE = os.path.join(HERE, "tiny_scene", "blender")
OUT = os.path.join(HERE, "grid_dataset.npz")
FACTORS = (1, 2, 3)
LR_STEPS = [0, 1, 2, 3, 7, 100, 1000, 7499, 7500, 15000, 15001, 38400, 128000, 250000, 250001, 400000]
LR_SETS = {      # lr_init, lr_final, delay_steps, delay_mult, max_steps
    "sigma": (3e1, 5e-2, 15000, 1e-2, 250000),
    "sh": (1e-2, 5e-6, 0, 1e-2, 250000),
    "short": (0.5, 0.125, 4, 0.1, 1000),
}


def import_reference():
    ref = os.environ.get("NERF_REFERENCE_SVOX2")
    if not ref or not os.path.isdir(os.path.join(ref, "opt", "util")):
        raise SystemExit("set NERF_REFERENCE_SVOX2 to the reference's svox2 directory")
    from PIL import Image
    imageio = types.ModuleType("imageio")
    imageio.imread = lambda path: np.asarray(Image.open(path)).copy()
    sys.modules["imageio"] = imageio
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sys.path.insert(0, os.path.join(ref, "opt"))
    from util import nerf_dataset, util      # noqa: E402  (the reference's)
    return nerf_dataset.NeRFDataset, util.get_expon_lr_func


def windows(full, small):
    return [((i * full) // small, -((-(i + 1) * full) // small)) for i in range(small)]


def exact(images_u8, c2w, fx, fy, cx, cy, factor):
    """(dirs, gt) in fp64."""
    n, H, W, _ = images_u8.shape
    h, w = H // factor, W // factor
    s = 1.0 / (H / h)
    u = (np.arange(w, dtype=np.float64) + 0.5 - cx * s) / (fx * s)
    v = (np.arange(h, dtype=np.float64) + 0.5 - cy * s) / (fy * s)
    d = np.stack(np.broadcast_arrays(u[None, :], v[:, None], np.ones((h, w))), -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    dirs = np.einsum("nrc,pc->npr", c2w[:, :3, :3].astype(np.float64), d.reshape(-1, 3)).reshape(-1, 3)
    q = images_u8.astype(np.float64) / 255.0
    q = q[..., :3] * q[..., 3:] + (1.0 - q[..., 3:])
    gt = np.zeros((n, h, w, 3))
    for y, (y0, y1) in enumerate(windows(H, h)):
        for x, (x0, x1) in enumerate(windows(W, w)):
            gt[:, y, x] = q[:, y0:y1, x0:x1].mean(axis=(1, 2))
    return dirs, gt.reshape(-1, 3)


def main():
    NeRFDataset, get_expon_lr_func = import_reference()
    torch.manual_seed(0)
    out = {}
    for f in FACTORS:
        ds = NeRFDataset(SCENE, "train", device="cpu", factor=f)
        r = ds.rays_init
        assert r.origins.dtype == torch.float32 and r.origins.shape == (3 * ds.h * ds.w, 3)
        out[f"origins_{f}"], out[f"dirs_{f}"], out[f"gt_{f}"] = r.origins.numpy(), r.dirs.numpy(), r.gt.numpy()
        out[f"hw_{f}"] = np.asarray([ds.h, ds.w], dtype=np.int64)
        if f == 1:
            it = ds.intrins_full
            out["c2w"] = ds.c2w.numpy().copy()
            out["intrins_full"] = np.asarray([it.fx, it.fy, it.cx, it.cy], dtype=np.float64)
            out["hw_full"] = np.asarray([ds.h_full, ds.w_full], dtype=np.int64)
            out["scene_scale"] = np.float64(ds.scene_scale)
            from PIL import Image
            import json
            frames = json.load(open(os.path.join(SCENE, "transforms_train.json")))["frames"]
            out["images_u8"] = np.stack([np.asarray(Image.open(os.path.join(SCENE, "train", os.path.basename(fr["file_path"])
                                                                            + ".png"))) for fr in frames])
            assert out["images_u8"].shape == (3, 16, 16, 4) and out["images_u8"].dtype == np.uint8
        assert np.array_equal(ds.c2w.numpy(), out["c2w"])
        dirs64, gt64 = exact(out["images_u8"], out["c2w"], *out["intrins_full"].tolist(), f)
        out[f"dirs64_{f}"], out[f"gt64_{f}"] = dirs64, gt64
        out[f"d_dirs_{f}"] = np.float64(np.abs(out[f"dirs_{f}"].astype(np.float64) - dirs64).max())
        out[f"d_gt_{f}"] = np.float64(np.abs(out[f"gt_{f}"].astype(np.float64) - gt64).max())
        print(f"factor {f}: {ds.h} x {ds.w}, reference fp32 vs fp64: dirs {out[f'd_dirs_{f}']:.3e}, gt {out[f'd_gt_{f}']:.3e}")
        assert out[f"d_dirs_{f}"] < 1e-6 and out[f"d_gt_{f}"] < 1e-6
    out["lr_steps"] = np.asarray(LR_STEPS, dtype=np.int64)
    for name, (lr0, lr1, delay, mult, steps) in LR_SETS.items():
        fn = get_expon_lr_func(lr0, lr1, delay, mult, steps)
        out[f"lr_{name}_args"] = np.asarray([lr0, lr1, delay, mult, steps], dtype=np.float64)
        out[f"lr_{name}"] = np.asarray([fn(s) for s in LR_STEPS], dtype=np.float64)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
