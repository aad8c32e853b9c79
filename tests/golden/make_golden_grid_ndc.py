"""Writes tests/golden/grid_ndc.npz: what the reference's svox2 gives for the forward-facing scene
tests/golden/tiny_scene/llff_svox2 (5 images of 16 x 24, read at scale 0.5 from images_2/: 8 x 12) - its LLFF loader, its NDC
rays, and a render of a small grid along them.

    NERF_REFERENCE_SVOX2=/path/to/reference/svox2 python tests/golden/make_golden_grid_ndc.py

Runs on the CPU in seconds. The reference's ``opt/util/llff_dataset.py`` and ``svox2`` are imported and run as they are;
``cv2`` and ``imageio`` are not installed, so stand-ins are put into ``sys.modules`` before the import: an ``imageio`` whose
``imread`` decodes with Pillow and an empty ``cv2`` (the loader calls it only for a scale without a pre-scaled folder).
Nothing of the reference is copied: the fixture holds arrays only.

(1) ``LLFFDataset(scene, "train", scale=0.5, offset=OFFSET)`` at factors 1 and 2: ``world_*`` = the rays of
    ``DatasetBase.gen_rays`` (before the warp), ``ndc_*`` = ``rays_init`` after ``LLFFDataset.gen_rays``, the ground truth,
    and ``c2w``, the intrinsics, ``ndc_coeffs``, ``scene_radius``, ``z_bounds``.
(2) The ``"test"`` split's ``c2w`` and ``render_c2w`` (and the train split's ``c2w``) at ``hold_every`` 8 and 2.
(3) ``svox2.Camera(..., ndc_coeffs).gen_rays()`` for the four training poses (cam0 .. cam3) and for one 13 x 9 camera with
    ``fx != fy`` and an off-centre principal point (cam4).
(4) For each of those the same formulas in fp64 (nothing rounded to fp32 on the way) and ``d_* = max |fp32 - fp64|``.
(5) ``SparseGrid._volume_render_gradcheck_lerp`` in fp32 and fp64 on the NDC rays of (1) at factor 1 and of cam4: a grid of
    ``reso [12, 10, 6]`` with the data set's ``scene_radius``, every node kept, random densities and SH,
    ``background_brightness = 0.5``; ``d_ref`` = the largest |fp32 - fp64|, from which the test takes its bar. The script
    asserts that in every recorded render at least half of the rays end with an opacity above 0.1 (the opacity is
    1 - (render over white - render over black), in fp64).
"""
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SCENE = os.path.join(HERE, "tiny_scene", "llff_svox2")
OUT = os.path.join(HERE, "grid_ndc.npz")
OFFSET = 6
RESO = (12, 10, 6)
BASIS_DIM = 9
CAM4 = dict(fx=9.7, fy=10.4, cx=6.9, cy=4.2, width=13, height=9)


def import_reference():
    ref = os.environ.get("NERF_REFERENCE_SVOX2")
    if not ref or not os.path.isdir(os.path.join(ref, "opt", "util")):
        raise SystemExit("set NERF_REFERENCE_SVOX2 to the reference's svox2 directory")
    from PIL import Image
    imageio = types.ModuleType("imageio")
    imageio.imread = lambda path, **kw: np.asarray(Image.open(path)).copy()
    sys.modules["imageio"] = imageio
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sys.path.insert(0, ref)
    sys.path.insert(0, os.path.join(ref, "opt"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import svox2      # noqa: E402  (the reference's)
        from util import dataset_base, llff_dataset      # noqa: E402
    return svox2, llff_dataset.LLFFDataset, dataset_base.DatasetBase


def ndc64(o, d, coeffs):
    """convert_to_ndc with near = 1 and the normalisation, in fp64."""
    t = (1.0 - o[:, 2]) / d[:, 2]
    o = o + t[:, None] * d
    oo = np.stack([coeffs[0] * (o[:, 0] / o[:, 2]), coeffs[1] * (o[:, 1] / o[:, 2]), 1.0 - 2.0 / o[:, 2]], -1)
    dd = np.stack([coeffs[0] * (d[:, 0] / d[:, 2] - o[:, 0] / o[:, 2]), coeffs[1] * (d[:, 1] / d[:, 2] - o[:, 1] / o[:, 2]),
                   2.0 / o[:, 2]], -1)
    return oo, dd / np.linalg.norm(dd, axis=-1, keepdims=True)


def world64(c2w, fx, fy, cx, cy, h, w):
    """The rays of every pose in fp64: pixel centres at + 0.5, normalise, rotate."""
    u = (np.arange(w, dtype=np.float64) + 0.5 - cx) / fx
    v = (np.arange(h, dtype=np.float64) + 0.5 - cy) / fy
    d = np.stack(np.broadcast_arrays(u[None, :], v[:, None], np.ones((h, w))), -1).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    c2w = c2w.astype(np.float64)
    dirs = np.einsum("nrc,pc->npr", c2w[:, :3, :3], d).reshape(-1, 3)
    origins = np.repeat(c2w[:, :3, 3], h * w, axis=0)
    return origins, dirs


def dist(a32, b64):
    return np.float64(np.abs(a32.astype(np.float64) - b64).max())


def ref_grid(svox2, radius, links, density, sh, dtype):
    g = svox2.SparseGrid(reso=[2, 2, 2], radius=list(radius), center=[0.0, 0.0, 0.0], basis_dim=BASIS_DIM, device="cpu")
    g.links = torch.from_numpy(links)
    g.density_data = torch.nn.Parameter(torch.from_numpy(density).to(dtype), requires_grad=False)
    g.sh_data = torch.nn.Parameter(torch.from_numpy(sh).to(dtype), requires_grad=False)
    g.capacity = density.shape[0]
    if dtype == torch.float64:
        g.radius = torch.tensor(np.array(radius, dtype=np.float32)).double()
        g.center = torch.zeros(3, dtype=torch.float64)
        g._offset = 0.5 * (1.0 - g.center / g.radius)
        g._scaling = 0.5 / g.radius

        def fetch64(self, lk):      # rows of the (double) data at the links, zeros at empty nodes
            present = (lk >= 0).unsqueeze(-1)
            rows = lk.clamp(min=0).long()
            zero = torch.zeros((), dtype=self.density_data.dtype)
            return torch.where(present, self.density_data[rows], zero), torch.where(present, self.sh_data[rows], zero)
        g._fetch_links = types.MethodType(fetch64, g)
    return g


def render(svox2, g, o, d, dt, bg):
    g.opt.background_brightness, g.opt.step_size, g.opt.near_clip = bg, 0.5, 0.0
    torch.set_default_dtype(dt)
    try:
        with torch.no_grad():
            rays = svox2.Rays(torch.from_numpy(o).to(dt), torch.from_numpy(d).to(dt))
            return g._volume_render_gradcheck_lerp(rays).numpy()
    finally:
        torch.set_default_dtype(torch.float32)


def main():
    svox2, LLFFDataset, DatasetBase = import_reference()
    out = {"offset": np.int64(OFFSET)}

    # (1) the training split: world rays, NDC rays, ground truth
    for f in (1, 2):
        ds = LLFFDataset(SCENE, "train", device="cpu", scale=0.5, offset=OFFSET, factor=f)
        DatasetBase.gen_rays(ds, f)
        world = ds.rays_init
        out[f"world_origins_{f}"], out[f"world_dirs_{f}"] = world.origins.numpy().copy(), world.dirs.numpy().copy()
        ds.gen_rays(f)
        r = ds.rays_init
        assert r.origins.dtype == torch.float32 and r.origins.shape == (ds.n_images * ds.h * ds.w, 3)
        out[f"ndc_origins_{f}"], out[f"ndc_dirs_{f}"], out[f"gt_{f}"] = r.origins.numpy(), r.dirs.numpy(), r.gt.numpy()
        out[f"hw_{f}"] = np.asarray([ds.h, ds.w], dtype=np.int64)
        it = ds.intrins
        out[f"intrins_{f}"] = np.asarray([it.fx, it.fy, it.cx, it.cy], dtype=np.float64)
        if f == 1:
            it = ds.intrins_full
            out["c2w"] = ds.c2w.numpy().copy()
            out["intrins_full"] = np.asarray([it.fx, it.fy, it.cx, it.cy], dtype=np.float64)
            out["hw_full"] = np.asarray([ds.h_full, ds.w_full], dtype=np.int64)
            out["ndc_coeffs"] = np.asarray(ds.ndc_coeffs, dtype=np.float64)
            out["scene_radius"] = np.asarray(ds.scene_radius, dtype=np.float64)
            out["z_bounds"] = np.asarray(ds.z_bounds, dtype=np.float64)
            assert ds.n_images == 4 and (ds.h_full, ds.w_full) == (8, 12) and not ds.use_sphere_bound
            from PIL import Image
            names = sorted(os.listdir(os.path.join(SCENE, "images_2")))
            out["images_u8"] = np.stack([np.asarray(Image.open(os.path.join(SCENE, "images_2", n))) for i, n in enumerate(names)
                                         if i % 8 > 0])
            assert out["images_u8"].shape == (4, 8, 12, 3) and out["images_u8"].dtype == np.uint8
        assert np.array_equal(ds.c2w.numpy(), out["c2w"])
        # (4) the same in fp64
        s = 1.0 / (ds.h_full / ds.h)
        fx, fy, cx, cy = (v * s for v in out["intrins_full"].tolist())
        o64, d64 = world64(out["c2w"], fx, fy, cx, cy, ds.h, ds.w)
        no64, nd64 = ndc64(o64, d64, out["ndc_coeffs"])
        out[f"ndc_origins64_{f}"], out[f"ndc_dirs64_{f}"] = no64, nd64
        out[f"d_origins_{f}"], out[f"d_dirs_{f}"] = dist(out[f"ndc_origins_{f}"], no64), dist(out[f"ndc_dirs_{f}"], nd64)
        print(f"factor {f}: {ds.h} x {ds.w}, reference fp32 vs fp64: origins {out[f'd_origins_{f}']:.3e}, dirs {out[f'd_dirs_{f}']:.3e}")
        assert out[f"d_origins_{f}"] < 1e-5 and out[f"d_dirs_{f}"] < 1e-5

    # (2) the splits
    for hold in (8, 2):
        for split in ("train", "test"):
            ds = LLFFDataset(SCENE, split, device="cpu", scale=0.5, offset=OFFSET, hold_every=hold)
            out[f"{split}_c2w_hold{hold}"] = ds.c2w.numpy().copy()
            out[f"{split}_z_bounds_hold{hold}"] = np.asarray(ds.z_bounds, dtype=np.float64)
            if split == "test":
                out[f"render_c2w_hold{hold}"] = ds.render_c2w.numpy().copy()
            print(f"hold_every {hold} {split}: {ds.n_images} views of {ds.h_full} x {ds.w_full}, z_bounds {ds.z_bounds}")

    # (3) cameras: the four training poses with the data set's intrinsics, and a 13 x 9 one
    ang = np.array([0.04, -0.07, 0.05])
    rx = np.array([[1, 0, 0], [0, np.cos(ang[0]), -np.sin(ang[0])], [0, np.sin(ang[0]), np.cos(ang[0])]])
    ry = np.array([[np.cos(ang[1]), 0, np.sin(ang[1])], [0, 1, 0], [-np.sin(ang[1]), 0, np.cos(ang[1])]])
    rz = np.array([[np.cos(ang[2]), -np.sin(ang[2]), 0], [np.sin(ang[2]), np.cos(ang[2]), 0], [0, 0, 1]])
    pose4 = out["c2w"][0][:3].astype(np.float64)
    pose4 = np.concatenate([(rz @ ry @ rx) @ pose4[:, :3], pose4[:, 3:] + np.array([[0.05], [-0.03], [0.02]])], 1).astype(np.float32)
    fx, fy, cx, cy = out["intrins_full"].tolist()
    cams = [dict(c2w=out["c2w"][i][:3], fx=fx, fy=fy, cx=cx, cy=cy, width=12, height=8, ndc=out["ndc_coeffs"].tolist()) for i in range(4)]
    cams.append(dict(c2w=pose4, ndc=[2 * CAM4["fx"] / CAM4["width"], 2 * CAM4["fy"] / CAM4["height"]], **CAM4))
    for i, c in enumerate(cams):
        cam = svox2.Camera(torch.from_numpy(np.ascontiguousarray(c["c2w"])), fx=c["fx"], fy=c["fy"], cx=c["cx"], cy=c["cy"],
                           width=c["width"], height=c["height"], ndc_coeffs=tuple(c["ndc"]))
        rays = cam.gen_rays()
        assert rays.origins.dtype == torch.float32
        out[f"cam{i}_c2w"] = np.ascontiguousarray(c["c2w"])
        out[f"cam{i}_intrinsics"] = np.array([c["fx"], c["fy"], c["cx"], c["cy"]])
        out[f"cam{i}_size"] = np.array([c["width"], c["height"]])
        out[f"cam{i}_ndc_coeffs"] = np.array(c["ndc"], dtype=np.float64)
        out[f"cam{i}_origins"], out[f"cam{i}_dirs"] = rays.origins.numpy(), rays.dirs.numpy()
        o64, d64 = world64(c["c2w"][None], c["fx"], c["fy"], c["cx"], c["cy"], c["height"], c["width"])
        no64, nd64 = ndc64(o64, d64, c["ndc"])
        out[f"cam{i}_origins64"], out[f"cam{i}_dirs64"] = no64, nd64
        out[f"cam{i}_d_origins"], out[f"cam{i}_d_dirs"] = dist(out[f"cam{i}_origins"], no64), dist(out[f"cam{i}_dirs"], nd64)
        print(f"cam{i}: fp32 vs fp64: origins {out[f'cam{i}_d_origins']:.3e}, dirs {out[f'cam{i}_d_dirs']:.3e}")

    # (5) a render along the NDC rays
    rng = np.random.default_rng(20240923)
    n = RESO[0] * RESO[1] * RESO[2]
    links = rng.permutation(n).astype(np.int32).reshape(RESO)
    density = (np.round(rng.uniform(-4.0, 40.0, (n, 1)) * 16) / 16).astype(np.float32)
    density[rng.random((n, 1)) < 0.1] = 0.0
    sh = (np.round(rng.normal(0.0, 1.0, (n, 3 * BASIS_DIM)) * 64) / 64).astype(np.float32)
    out.update({"grid_links": links, "grid_density": density, "grid_sh": sh, "grid_reso": np.asarray(RESO, dtype=np.int64)})
    radius = out["scene_radius"].tolist()
    g32 = ref_grid(svox2, radius, links, density, sh, torch.float32)
    g64 = ref_grid(svox2, radius, links, density, sh, torch.float64)
    d_ref = 0.0
    for tag, o, d in (("train", out["ndc_origins_1"], out["ndc_dirs_1"]), ("cam4", out["cam4_origins"], out["cam4_dirs"])):
        rgb32 = render(svox2, g32, o, d, torch.float32, 0.5)
        rgb64 = render(svox2, g64, o, d, torch.float64, 0.5)
        assert rgb32.dtype == np.float32 and rgb64.dtype == np.float64
        opacity = 1.0 - (render(svox2, g64, o, d, torch.float64, 1.0) - render(svox2, g64, o, d, torch.float64, 0.0))[:, 0]
        share = float((opacity > 0.1).mean())
        out[f"render_{tag}_rgb"], out[f"render_{tag}_rgb64"], out[f"render_{tag}_opacity64"] = rgb32, rgb64, opacity
        d_ref = max(d_ref, float(np.abs(rgb32.astype(np.float64) - rgb64).max()))
        print(f"render {tag}: {len(o)} rays, opacity > 0.1 on {100 * share:.0f} %, |fp32 - fp64| max "
              f"{np.abs(rgb32.astype(np.float64) - rgb64).max():.3e}")
        assert share >= 0.5, f"render {tag}: only {100 * share:.0f} % of the rays end with opacity above 0.1: raise OFFSET"
    out["render_d_ref"] = np.float64(d_ref)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
