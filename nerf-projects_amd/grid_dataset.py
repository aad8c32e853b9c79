"""Training data for a sparse voxel grid (Plenoxels): the images stay on the GPU as they were loaded and every batch of rays
is made by one HIP launch (csrc/grid_dataset_kernels.hip; semantics: include/nerf_mi355x.h, "Sparse voxel grid: training
data").

``GridDataset`` has the surface of svox2's ``DatasetBase`` / ``NeRFDataset`` (``opt/util/dataset_base.py``,
``opt/util/nerf_dataset.py``) on another design. svox2's ``gen_rays`` materialises origin, direction and colour of every
pixel of every image (36 B per ray) and ``shuffle_rays`` copies all of them through a host ``randperm`` once per epoch. Here
``gen_rays`` only sets the factor, ``shuffle_rays`` only draws a 64-bit key, and ``batch(begin, end)`` asks the kernel for
rows ``[begin, end)`` of the epoch: row ``k`` is the ray ``sigma(k)``, an integer bijection keyed by the epoch (a random draw
without ``permutation``), whose direction and ground-truth colour are computed from the pose and the uint8 pixels. The
mapping::

    svox2                                   here
    NeRFDataset(root, split="train", ...)   GridDataset.from_blender(root, "train", ...)
    dset.gen_rays(factor)                   dset.gen_rays(factor)           (materialises nothing)
    dset.shuffle_rays()                     dset.shuffle_rays()             (a new key from dset.generator)
    dset.rays.origins[b:e], .dirs[b:e]      rays, rgb_gt = dset.batch(b, e)
    dset.rays.gt[b:e]
    dset.rays.origins.size(0)               dset.n_rays
    svox2.Camera(dset.c2w[i], ...)          dset.camera(i)                  (an NdcCamera where dset.ndc_coeffs are set)
    dset.gt[i]                              dset.image(i)
    LLFFDataset(root, split="train", ...)   GridDataset.from_llff(root, "train", ...)

The rays of a batch are those of svox2 for the same ray index (directions to the last bit on the committed scene, colours
too); WHICH ray comes at which position of an epoch is this package's ``sigma``, not ``torch.randperm``'s. A forward-facing
(LLFF) scene carries ``ndc_coeffs``: the batch kernel then sends every world ray through the NDC warp (``rays_to_ndc`` in
csrc/grid_device.h, svox2's ``convert_to_ndc`` and the normalisation after it), and ``camera(i)`` is an ``NdcCamera``. Not
offered: the NSVF and CO3D loaders. There is no CPU or PyTorch fallback.
"""
import ctypes as C
import json
import os
from dataclasses import dataclass

import numpy as np
import torch

from ._lib import (NERF_GRID_ORDER_IDENTITY, NERF_GRID_ORDER_PERMUTED, NERF_GRID_ORDER_RANDOM, GridDatasetBatchArgs, check)
from . import datasets
from .datasets import read_image
from .grid import Camera, NdcCamera, Rays, _ndc_coeffs_arg
from .host import get_context

__all__ = ["GridDataset", "Intrin"]

MAX_BATCH = 1 << 26      # rays per launch (include/nerf_mi355x.h)


@dataclass
class Intrin:
    """svox2's ``Intrin``: one set of intrinsics for every image."""
    fx: float
    fy: float
    cx: float
    cy: float

    def scale(self, scaling: float):
        return Intrin(self.fx * scaling, self.fy * scaling, self.cx * scaling, self.cy * scaling)

    def get(self, field: str, image_id: int = 0):
        return getattr(self, field)


def _images_arg(images_u8, device):
    if isinstance(images_u8, np.ndarray):
        if images_u8.dtype != np.uint8:
            raise TypeError(f"images_u8 must be uint8, got {images_u8.dtype}")
        t = torch.from_numpy(np.ascontiguousarray(images_u8))
    elif torch.is_tensor(images_u8):
        if not images_u8.is_cuda:
            raise RuntimeError("images_u8 is a CPU tensor: pass a numpy array (it is uploaded) or a device tensor; the batches "
                               "have no CPU fallback")
        if images_u8.dtype != torch.uint8:
            raise TypeError(f"images_u8 must be uint8, got {images_u8.dtype}")
        t = images_u8.detach()
    else:
        raise TypeError("images_u8 must be a uint8 numpy array or device tensor [n_images, H, W, 3 or 4]")
    if t.dim() != 4 or t.shape[3] not in (3, 4) or min(t.shape[:3]) < 1:
        raise ValueError(f"images_u8 must be [n_images, H, W, 3 or 4], got {tuple(t.shape)}")
    return t.to(device).contiguous()


def _c2w_arg(c2w, n_images):
    """fp32 CPU ``[n, 4, 4]`` from ``[n, 3, 4]`` or ``[n, 4, 4]``."""
    m = torch.as_tensor(np.asarray(c2w.detach().cpu()) if torch.is_tensor(c2w) else np.asarray(c2w))
    if not m.dtype.is_floating_point:
        raise TypeError(f"c2w must be floating point, got {m.dtype}")
    if m.dim() != 3 or m.shape[0] != n_images or tuple(m.shape[1:]) not in ((3, 4), (4, 4)):
        raise ValueError(f"c2w must be [{n_images}, 3, 4] or [{n_images}, 4, 4] like the images, got {tuple(m.shape)}")
    m = m.to(torch.float32)
    if not bool(torch.isfinite(m).all()):
        raise ValueError("c2w is not finite")
    full = torch.zeros((n_images, 4, 4), dtype=torch.float32)
    full[:, 3, 3] = 1.0
    full[:, :3] = m[:, :3]
    return full


def _mean_frame(poses):
    """load_llff.py's ``poses_avg`` for ``[n, 3, 4]`` poses: the 3 x 4 frame of the mean camera."""
    return datasets.viewmatrix(poses[:, :, 2].sum(0), poses[:, :, 1].sum(0), poses[:, :, 3].mean(0))


def _llff_c2w(poses):
    """svox2's ``nerf_pose_to_ours`` on fp32 ``[n, 3, 4]`` poses ``[right | up | back | position]``: the y and z components
    of the position negated, and of the rotation the entries ``[1:, 0]`` and ``[0, 1:]``. fp32 ``[n, 4, 4]``."""
    out = torch.zeros((len(poses), 4, 4), dtype=torch.float32)
    m = np.array(poses, dtype=np.float32)
    m[:, 1:, 3] *= -1
    m[:, 1:, 0] *= -1
    m[:, 0, 1:3] *= -1
    out[:, :3] = torch.from_numpy(m)
    out[:, 3, 3] = 1.0
    return out


class GridDataset:
    """The training (or test) views of one scene, resident on the GPU as ``images_u8`` ``[n_images, H, W, C]`` and poses.

    ``c2w`` ``[n_images, 4, 4]`` (OpenCV convention, on the device), ``n_images``, ``h_full``, ``w_full``, ``intrins_full``,
    ``h``, ``w``, ``intrins`` (at the current factor), ``ndc_coeffs`` (``(-1, -1)``, or the two positive coefficients of a
    forward-facing scene given as ``ndc_coeffs=``), ``scene_center``, ``scene_radius``,
    ``use_sphere_bound``, ``split``, ``permutation``, ``epoch_size`` as in svox2's ``DatasetBase``. ``generator``: the CPU
    ``torch.Generator`` that :meth:`shuffle_rays` draws the epoch keys from."""

    def __init__(self, images_u8, c2w, fx, fy, cx, cy, split="train", white_bkgd=True, n_images=None, epoch_size=None,
                 permutation=True, device="cuda", generator=None, factor=1, ndc_coeffs=None):
        if torch.device(device).type != "cuda":
            raise RuntimeError(f"device {device} is not a GPU: GridDataset has no CPU fallback")
        self.ctx = get_context(device)
        self.device = self.ctx.device
        images = _images_arg(images_u8, self.device)
        poses = _c2w_arg(c2w, images.shape[0])
        if n_images is not None:
            if not isinstance(n_images, (int, np.integer)) or n_images < 1:
                raise ValueError(f"n_images = {n_images!r} must be a positive int")
            n_images = min(int(n_images), images.shape[0])      # (svox2 uses what there is)
            images, poses = images[:n_images].contiguous(), poses[:n_images]
        for name, v, positive in (("fx", fx, True), ("fy", fy, True), ("cx", cx, False), ("cy", cy, False)):
            if not np.isfinite(v) or (positive and not v > 0):
                raise ValueError(f"{name} = {v!r} must be finite" + (" and positive" if positive else ""))
        if epoch_size is not None and (not isinstance(epoch_size, (int, np.integer)) or epoch_size < 1):
            raise ValueError(f"epoch_size = {epoch_size!r} must be a positive int or None")
        self.images_u8 = images
        self.c2w = poses.to(self.device)
        self._poses = self.c2w[:, :3, :].reshape(-1, 12).contiguous()
        self.n_images, self.h_full, self.w_full, self.channels = (int(s) for s in images.shape)
        self.intrins_full = Intrin(float(fx), float(fy), float(cx), float(cy))
        self.split = split
        self.white_bkgd = bool(white_bkgd)
        self.permutation = bool(permutation)
        self.epoch_size = None if epoch_size is None else int(epoch_size)
        self.generator = generator if generator is not None else torch.Generator(device="cpu")
        self.ndc_coeffs = (-1, -1) if ndc_coeffs is None else tuple(_ndc_coeffs_arg(ndc_coeffs))
        self.use_sphere_bound = True
        self.should_use_background = False
        self.scene_center = [0.0, 0.0, 0.0]
        self.scene_radius = [1.0, 1.0, 1.0]
        self.key = 0
        self._shuffled = False      # as svox2's rays = rays_init: the index order until the first shuffle_rays()
        self.gen_rays(factor)

    # ---- constructors ---------------------------------------------------------------------------------------------------
    @classmethod
    def from_arrays(cls, images_u8, c2w, fx, fy, cx, cy, split="train", white_bkgd=True, n_images=None, epoch_size=None,
                    permutation=True, device="cuda", generator=None, ndc_coeffs=None):
        """``images_u8``: uint8 ``[n_images, H, W, 3 or 4]``, a numpy array (uploaded) or a device tensor (borrowed);
        ``c2w``: ``[n_images, 3, 4]`` or ``[n_images, 4, 4]`` camera-to-world in the OpenCV convention; ``fx, fy, cx, cy``
        of the full-resolution images; ``ndc_coeffs``: ``(2 fx / W, 2 fy / H)`` for a forward-facing scene whose rays are
        to be warped to NDC, else ``None``."""
        return cls(images_u8, c2w, fx, fy, cx, cy, split, white_bkgd, n_images, epoch_size, permutation, device, generator,
                   ndc_coeffs=ndc_coeffs)

    @classmethod
    def from_blender(cls, root, split, scene_scale=2 / 3, white_bkgd=True, n_images=None, epoch_size=None, permutation=True,
                     device="cuda", generator=None):
        """A NeRF-synthetic (Blender) scene directory as svox2's ``NeRFDataset`` reads it: ``transforms_<split>.json`` and
        the PNGs it names (``"test_train"`` reads the train split), poses flipped from OpenGL to OpenCV by
        ``c2w @ diag(1, -1, -1, 1)``, translations times ``scene_scale``, focal length from ``camera_angle_x``, principal
        point at the image centre."""
        if not os.path.isdir(root):
            raise FileNotFoundError(f"'{root}' is not a directory")
        name = "train" if split == "test_train" else split
        with open(os.path.join(root, f"transforms_{name}.json")) as f:
            meta = json.load(f)
        flip = torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0], dtype=torch.float32))
        images, poses = [], []
        for frame in meta["frames"]:
            images.append(read_image(os.path.join(root, name, os.path.basename(frame["file_path"]) + ".png")))
            poses.append(torch.tensor(frame["transform_matrix"], dtype=torch.float32) @ flip)
        if not images:
            raise ValueError(f"transforms_{name}.json names no frame")
        images = np.stack(images)
        if images.ndim != 4:
            raise ValueError(f"the images of {root} are {images.shape[1:]}: RGB or RGBA expected")
        c2w = torch.stack(poses)
        c2w[:, :3, 3] *= 2 / 3 if scene_scale is None else scene_scale
        w = images.shape[2]
        focal = float(0.5 * w / np.tan(0.5 * meta["camera_angle_x"]))
        ds = cls(images, c2w, focal, focal, w * 0.5, images.shape[1] * 0.5, split, white_bkgd, n_images, epoch_size,
                 permutation, device, generator)
        ds.scene_scale = 2 / 3 if scene_scale is None else scene_scale
        return ds

    @classmethod
    def from_llff(cls, root, split, scale=None, hold_every=8, offset=250, n_images=None, epoch_size=None, permutation=True,
                  device="cuda", generator=None):
        """A forward-facing (LLFF) scene directory as svox2's ``LLFFDataset`` reads it (``opt/util/llff_dataset.py`` with
        ``SfMData.readLLFF`` and ``opt/util/load_llff.py``): poses, depth bounds and ``(H, W, focal)`` from
        ``poses_bounds.npy``; translations scaled so that the nearest bound is ``1 / 0.75``; poses recentred on their mean
        camera and turned to the OpenCV convention (``nerf_pose_to_ours``); intrinsics scaled by ``scale`` (default 1/4) as
        ``scaleAll`` does; image ``i`` (files of the folder in name order) is a training view iff ``i % hold_every > 0``, a
        split whose name ends in ``"train"`` takes those and any other split the rest.

        Sets ``ndc_coeffs = (2 fx / w_full, 2 fy / h_full)``, so that batches and cameras are in NDC;
        ``scene_radius = [1 + 2 offset / w, 1 + 2 offset / h, 1]`` (``offset`` pixels of padding around the reference view),
        ``scene_center = 0``, ``use_sphere_bound = False``, ``white_bkgd = False``, ``z_bounds`` (the scaled depth bounds of
        the training view nearest the mean camera; not used, as in svox2) and, for a test split, ``render_c2w``
        ``[120, 4, 4]``: the spiral path.

        Images: ``images/`` at ``scale == 1``; ``images_<1/scale>/`` when ``1 / scale`` is an integer and that folder
        exists. Any other scaling is ``cv2.resize(..., INTER_AREA)`` in svox2, which this package does not have: it raises.
        Not read: ``hwf_cxcy.npy``, ``planes.txt``, ``bounds.txt`` (NeX's extensions)."""
        if not os.path.isdir(root):
            raise FileNotFoundError(f"'{root}' is not a directory")
        scale = 0.25 if scale is None else float(scale)
        if not np.isfinite(scale) or not scale > 0:
            raise ValueError(f"scale = {scale!r} must be positive and finite")
        if not isinstance(hold_every, (int, np.integer)) or hold_every < 1:
            raise ValueError(f"hold_every = {hold_every!r} must be a positive int")
        for extension in ("hwf_cxcy.npy", "planes.txt", "bounds.txt"):
            if os.path.exists(os.path.join(root, extension)):
                raise NotImplementedError(f"{extension} in {root}: NeX's extensions of the LLFF format are not read")
        image_dir = "images"
        if scale != 1:
            inverse = round(1.0 / scale)
            if abs(1.0 / scale - inverse) >= 1e-9 or not os.path.isdir(os.path.join(root, f"images_{inverse}")):
                raise NotImplementedError(
                    f"scale = {scale}: svox2 resizes the images with cv2.INTER_AREA here, which this package does not have. "
                    f"Give a scale whose inverse is an integer k and provide the folder images_k (e.g. made with ImageMagick: "
                    f"mogrify -resize {100.0 * scale:g}% -format png), or scale = 1")
            image_dir = f"images_{inverse}"

        arr = np.load(os.path.join(root, "poses_bounds.npy"))
        if arr.ndim != 2 or arr.shape[1] != 17:
            raise ValueError(f"poses_bounds.npy is {arr.shape}, expected [n, 17]")
        blocks = arr[:, :15].reshape(-1, 3, 5)
        H, W, focal = (float(v) for v in blocks[0, :, 4])
        # LLFF stores the rotation columns as [down, right, back]; load_llff.py wants [right, up, back]
        poses = np.concatenate([blocks[:, :, 1:2], -blocks[:, :, 0:1], blocks[:, :, 2:4]], 2).astype(np.float32)
        bds = arr[:, 15:].astype(np.float32)
        sc = 1.0 / (bds.min() * 0.75)
        poses[:, :, 3] *= sc
        bds *= sc
        poses = datasets._into_frame(_mean_frame(poses), poses).astype(np.float32)      # recenter_poses
        names = [f for f in os.listdir(os.path.join(root, image_dir))
                 if not f.startswith(".") and f.lower().endswith((".png", ".jpg", ".jpeg"))]
        names.sort(key=lambda f: f[2:] if len(f) > 2 and f[1] == "_" else f)      # svox2's NSVF-compatible sort key
        if len(names) != len(poses):
            raise ValueError(f"{len(names)} images in {image_dir}/ but {len(poses)} poses in poses_bounds.npy")

        held = np.arange(len(poses)) % hold_every == 0
        is_train = split.endswith("train")
        pick = np.flatnonzero(~held if is_train else held)
        if pick.size == 0:
            raise ValueError(f"hold_every = {hold_every} leaves no view in the {split!r} split of {len(poses)} images")
        if not (~held).any():
            raise ValueError(f"hold_every = {hold_every} leaves no training view (the depth bounds come from one)")
        # the depth bounds of the training view nearest the mean training camera
        train = poses[~held]
        nearest = int(np.argmin(np.sum(np.square(_mean_frame(train)[:, 3] - train[:, :, 3]), -1)))
        z_bounds = [float(v) for v in bds[~held][nearest]]

        # scaleAll: the scaled size is rounded, each axis scales by its own ratio
        w_ref, h_ref = int(W), int(H)
        nw, nh = round(w_ref * scale), round(h_ref * scale)
        sw, sh = nw / w_ref, nh / h_ref
        fx, fy, cx, cy = focal * sw, focal * sh, (W / 2.0) * sw, (H / 2.0) * sh

        images = np.stack([read_image(os.path.join(root, image_dir, names[i])) for i in pick])
        if images.ndim != 4 or images.shape[3] != 3:
            raise ValueError(f"the images of {root}/{image_dir} are {images.shape[1:]}: RGB expected (svox2 composites an alpha "
                             "channel over white: from_arrays(..., white_bkgd=True, ndc_coeffs=...) does that)")
        if images.shape[1:3] != (nh, nw):
            raise ValueError(f"the images of {image_dir}/ are {images.shape[1]} x {images.shape[2]}, poses_bounds.npy and scale "
                             f"= {scale} say {nh} x {nw}")
        ds = cls(images, _llff_c2w(poses[pick]), fx, fy, cx, cy, split, False, n_images, epoch_size, permutation, device,
                 generator, ndc_coeffs=(2.0 * fx / nw, 2.0 * fy / nh))
        ds.scale, ds.hold_every, ds.offset = scale, int(hold_every), offset
        ds.z_bounds = z_bounds
        ds.scene_center = [0.0, 0.0, 0.0]
        ds.scene_radius = [1 + 2 * offset / nw, 1 + 2 * offset / nh, 1.0]
        ds.use_sphere_bound = False
        if not is_train:
            # load_llff.py's spiral: two turns of 120 views around the mean camera, looking at the focus depth
            frame = _mean_frame(poses)
            up = datasets.normalize(poses[:, :, 1].sum(0))
            close_depth, inf_depth = bds.min() * 0.9, bds.max() * 5.0
            focus = 1.0 / (0.25 / close_depth + 0.75 / inf_depth)
            rads = np.percentile(np.abs(poses[:, :, 3]), 90, 0)
            path = datasets.render_path_spiral(np.concatenate([frame, np.zeros((3, 1))], 1), up, rads, focus, 0.0, zrate=0.5,
                                               rots=2, N=120)
            ds.render_c2w = _llff_c2w(np.asarray(path)[:, :, :4].astype(np.float32)).to(ds.device)
        return ds

    # ---- svox2's surface ------------------------------------------------------------------------------------------------
    def gen_rays(self, factor=1):
        """Sets the down-sampling factor: ``h = h_full // factor``, ``w = w_full // factor``, the intrinsics times
        ``h / h_full``. Nothing is materialised; the colours of a factor above 1 are area means made in the batch kernel."""
        if not isinstance(factor, (int, np.integer)) or isinstance(factor, bool) or not 1 <= factor <= min(self.h_full, self.w_full):
            raise ValueError(f"factor = {factor!r} must be an int in [1, {min(self.h_full, self.w_full)}]")
        self.factor = int(factor)
        self.h, self.w = self.h_full // self.factor, self.w_full // self.factor
        self.intrins = self.intrins_full.scale(1.0 / (self.h_full / self.h))

    def shuffle_rays(self):
        """A new epoch: draws the 64-bit key of its order from ``self.generator`` (train split only, as svox2). Nothing moves."""
        if self.split == "train":
            hi, lo = torch.randint(0, 1 << 32, (2,), generator=self.generator, dtype=torch.int64).tolist()
            self.key = (hi << 32) | lo
            self._shuffled = True

    def get_image_size(self, i: int):
        return self.h, self.w

    @property
    def n_rays_full(self):
        return self.n_images * self.h * self.w

    @property
    def n_rays(self):
        """Rays of an epoch: all of them, or ``epoch_size`` (at most all of them under ``permutation``)."""
        if self.epoch_size is None or not self._shuffled:
            return self.n_rays_full
        return min(self.epoch_size, self.n_rays_full) if self.permutation else self.epoch_size

    @property
    def bytes_resident(self):
        return self.images_u8.numel() + 4 * self._poses.numel()

    def _order(self):
        if not self._shuffled:
            return NERF_GRID_ORDER_IDENTITY
        return NERF_GRID_ORDER_PERMUTED if self.permutation else NERF_GRID_ORDER_RANDOM

    def _launch(self, order, begin, n, want_indices):
        dev = self.device
        o = torch.empty((n, 3), dtype=torch.float32, device=dev)
        d = torch.empty((n, 3), dtype=torch.float32, device=dev)
        rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
        idx = torch.empty((n,), dtype=torch.int64, device=dev) if want_indices else None
        a = GridDatasetBatchArgs()
        a.images, a.c2w = self.images_u8.data_ptr(), self._poses.data_ptr()
        a.n_images, a.height, a.width, a.channels = self.n_images, self.h_full, self.w_full, self.channels
        it = self.intrins_full
        a.fx, a.fy, a.cx, a.cy = it.fx, it.fy, it.cx, it.cy
        a.white_bkgd, a.factor, a.order, a.key = int(self.white_bkgd), self.factor, order, self.key
        a.begin, a.n = begin, n
        a.origins, a.dirs, a.rgb = o.data_ptr(), d.data_ptr(), rgb.data_ptr()
        a.indices = None if idx is None else idx.data_ptr()
        a.stream = self.ctx.stream().value
        a.ndc_coeffs[:] = [float(v) for v in self.ndc_coeffs]
        check(self.ctx.lib.nerf_grid_dataset_batch(self.ctx.handle, C.byref(a)))
        return o, d, rgb, idx

    def batch(self, begin, end, return_indices=False):
        """``(Rays, rgb_gt)`` of rows ``[begin, end)`` of the current epoch, each ``[end - begin, 3]`` fp32 on the device,
        from one launch; with ``return_indices`` also the int64 ray index ``(image * h + y) * w + x`` of every row."""
        for name, v in (("begin", begin), ("end", end)):
            if not isinstance(v, (int, np.integer)) or isinstance(v, bool):
                raise TypeError(f"{name} = {v!r} must be an int")
        n_rays = self.n_rays
        if not 0 <= begin <= n_rays:
            raise ValueError(f"begin = {begin} outside the epoch [0, {n_rays}]")
        if not begin <= end <= n_rays:
            raise ValueError(f"end = {end} outside [begin, the epoch's end] = [{begin}, {n_rays}]")
        if end - begin > MAX_BATCH:
            raise ValueError(f"end - begin = {end - begin}: a batch holds at most 2^26 rays")
        o, d, rgb, idx = self._launch(self._order(), int(begin), int(end - begin), return_indices)
        return (Rays(o, d), rgb, idx) if return_indices else (Rays(o, d), rgb)

    def camera(self, i):
        """The ``Camera`` of image ``i`` at the current factor (what svox2's training script builds from ``dset.c2w[i]`` and
        ``dset.intrins``); an ``NdcCamera`` where the data set has ``ndc_coeffs``."""
        i = self._image_index(i)
        it = self.intrins
        kind = NdcCamera if self.ndc_coeffs[0] > 0 else Camera
        return kind(self.c2w[i], it.fx, it.fy, it.cx, it.cy, width=self.w, height=self.h, ndc_coeffs=self.ndc_coeffs)

    def image(self, i):
        """Ground truth ``[h, w, 3]`` of image ``i`` at the current factor: the batch kernel in index order (svox2's ``gt[i]``)."""
        i = self._image_index(i)
        hw = self.h * self.w
        if hw > MAX_BATCH:
            raise ValueError(f"an image of {self.h} x {self.w} exceeds the 2^26 rays of one launch")
        return self._launch(NERF_GRID_ORDER_IDENTITY, i * hw, hw, False)[2].view(self.h, self.w, 3)

    def _image_index(self, i):
        if not isinstance(i, (int, np.integer)) or isinstance(i, bool):
            raise TypeError(f"i = {i!r} must be an int")
        if not 0 <= i < self.n_images:
            raise IndexError(f"i = {i} outside [0, {self.n_images})")
        return int(i)
