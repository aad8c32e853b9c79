"""Sparse voxel grid with background layers: ``BackgroundGrid``, a ``SparseGrid`` that also carries svox2's multi-sphere-image
background (``background_nlayers`` concentric equirectangular layers around the grid) and renders it, as the checkpoints of
the Tanks-and-Temples, CO3D and custom configurations need.

``load_grid(path)`` opens any svox2 ``.npz``: a ``BackgroundGrid`` when the file has ``background_data``, else a
``SparseGrid``. The background is rendered by a HIP kernel of its own after the foreground (include/nerf_mi355x.h, "Sparse
voxel grid: background layers": the semantics of the reference's CUDA kernel, not of its PyTorch renderer) and can be thinned
on the device with :meth:`BackgroundGrid.sparsify_background`. As everywhere in this package there is no CPU or PyTorch
fallback.

Training it is ``grid_background_train.BackgroundTrainer``. ``GridTrainer``, ``GridModule``, ``resample_grid``,
``remove_floaters`` and ``to_half`` handle a foreground only and raise a ``NotImplementedError`` that names
:meth:`BackgroundGrid.foreground`, the ``SparseGrid`` on the same tensors.
"""
import ctypes as C
from dataclasses import replace
from typing import List, Tuple, Union

import numpy as np
import torch

from ._lib import (GridBackgroundArgs, GridBackgroundDesc, GridBackgroundGatherArgs, GridBackgroundSparsifyArgs, GridRenderArgs,
                   check)
from .grid import BASIS_TYPE_SH, NdcCamera, SparseGrid
from .host import get_context

__all__ = ["BackgroundGrid", "load_grid"]


def _check_nlayers_reso(nlayers, reso):
    nlayers, reso = int(nlayers), int(reso)
    if nlayers < 2 or nlayers > 1024:
        raise ValueError(f"background_nlayers = {nlayers}: at least 2 layers (the interpolation needs two) and at most 1024")
    if reso < 2 or reso > 1024:
        raise ValueError(f"background_reso = {reso} must be in [2, 1024]")
    return nlayers, reso


class BackgroundGrid(SparseGrid):
    """svox2.SparseGrid with ``background_nlayers > 0``, forward side. On top of a ``SparseGrid``'s tensors:
    ``background_links`` int32 ``[2 R, R]`` (``>= 0``: row of the data, negative: empty texel) and ``background_data`` fp32
    ``[capacity, L, 4]`` (colour, colour, colour, sigma), both on the GPU and borrowed by the C library. Assigning either, or
    writing into ``background_links`` in place, re-attaches the background before the next call (the version-counter rule of
    ``links``); the foreground's skip data is not touched by that.

    ``volume_render`` and ``volume_render_image`` include the background. Everything else is foreground-only, as in svox2,
    and inherited unchanged: ``volume_render_depth`` / ``_image``, ray lengths (``return_raylen``), ``sample``, ``accelerate``,
    ``count_samples``, ``compute_FDR``, ``label_components`` and the floater views."""

    def __init__(self, reso: Union[int, List[int], Tuple[int, int, int]] = 128, radius: Union[float, List[float]] = 1.0,
                 center: Union[float, List[float]] = [0.0, 0.0, 0.0], basis_type: int = BASIS_TYPE_SH, basis_dim: int = 9,
                 basis_reso: int = 16, use_z_order: bool = False, use_sphere_bound: bool = False, mlp_posenc_size: int = 0,
                 mlp_width: int = 16, background_nlayers: int = 0, background_reso: int = 256,
                 device: Union[torch.device, str] = "cuda"):
        if not background_nlayers:
            raise ValueError("BackgroundGrid needs background_nlayers >= 2 (and background_reso): without a background, SparseGrid")
        L, R = _check_nlayers_reso(background_nlayers, background_reso)
        super().__init__(reso, radius, center, basis_type, basis_dim, basis_reso, use_z_order, use_sphere_bound, mlp_posenc_size,
                         mlp_width, 0, background_reso, device)
        dev = self.ctx.device
        self._bg_key = None
        self._bg_links = torch.arange(2 * R * R, dtype=torch.int32, device=dev).view(2 * R, R)
        self._bg_data = torch.zeros((2 * R * R, L, 4), dtype=torch.float32, device=dev)
        self._bg_shape()

    @classmethod
    def from_tensors(cls, links, density_data, sh_data, radius, center, basis_dim=None, background_links=None,
                     background_data=None):
        """A grid around existing device tensors (all borrowed): those of ``SparseGrid.from_tensors`` and ``background_links``
        int32 ``[2 R, R]``, ``background_data`` fp32 ``[capacity, L, 4]``."""
        if background_links is None or background_data is None:
            raise ValueError("BackgroundGrid.from_tensors needs background_links and background_data: without a background, "
                             "SparseGrid.from_tensors")
        g = cls.__new__(cls)
        links = torch.as_tensor(links)
        if links.dim() != 3:
            raise ValueError(f"links must be [X, Y, Z], got shape {tuple(links.shape)}")
        if not links.is_cuda:
            raise RuntimeError("links is on the CPU: BackgroundGrid has no CPU fallback (pass device tensors)")
        sh_data = torch.as_tensor(sh_data)
        if sh_data.dim() != 2 or sh_data.shape[1] % 3:
            raise ValueError(f"sh_data must be [capacity, 3 * basis_dim], got shape {tuple(sh_data.shape)}")
        bd = sh_data.shape[1] // 3 if basis_dim is None else basis_dim
        g._init_common(list(links.shape), radius, center, BASIS_TYPE_SH, bd, 0, links.device)
        g.capacity = int(sh_data.shape[0])
        g._links, g._density, g._sh = links, torch.as_tensor(density_data), sh_data
        g._bg_key = None
        g._bg_links, g._bg_data = background_links, background_data
        g._handle()      # validates
        return g

    @classmethod
    def from_grid(cls, grid: SparseGrid, background_nlayers: int, background_reso: int = 256):
        """``grid`` with a fresh background (every texel has a row, all zeros): the foreground tensors are shared with
        ``grid``, ``opt`` is a copy."""
        if not isinstance(grid, SparseGrid) or getattr(grid, "is_half", False) or getattr(grid, "is_palette", False):
            raise TypeError("BackgroundGrid.from_grid needs a SparseGrid (fp32 colours)")
        L, R = _check_nlayers_reso(background_nlayers, background_reso)
        dev = grid.ctx.device
        g = cls.from_tensors(grid.links, grid.density_data, grid.sh_data, grid.radius, grid.center, basis_dim=grid.basis_dim,
                             background_links=torch.arange(2 * R * R, dtype=torch.int32, device=dev).view(2 * R, R),
                             background_data=torch.zeros((2 * R * R, L, 4), dtype=torch.float32, device=dev))
        g.opt = replace(grid.opt)
        return g

    def foreground(self) -> SparseGrid:
        """The ``SparseGrid`` on the same ``links``, ``density_data`` and ``sh_data`` (shared, not copied), with a copy of
        ``opt``: what trains, resamples and loses its floaters."""
        g = SparseGrid.from_tensors(self._links, self._density, self._sh, self.radius, self.center, basis_dim=self.basis_dim)
        g.opt = replace(self.opt)
        return g

    # ---- the borrowed tensors -------------------------------------------------------------------------------
    def _drop_handle(self):
        super()._drop_handle()
        self._bg_key = None      # a new handle has no background attached

    __del__ = _drop_handle

    def _bg_shape(self):
        L, D = self._bg_links, self._bg_data
        if torch.is_tensor(L) and L.dim() == 2:
            self.background_reso = int(L.shape[1])
        if torch.is_tensor(D) and D.dim() == 3:
            self.background_nlayers = int(D.shape[1])

    @property
    def background_links(self):
        return self._bg_links

    @background_links.setter
    def background_links(self, t):
        self._bg_key = None
        self._bg_links = t
        self._bg_shape()

    @property
    def background_data(self):
        return self._bg_data

    @background_data.setter
    def background_data(self, t):
        self._bg_key = None
        self._bg_data = t
        self._bg_shape()

    @property
    def use_background(self):
        return True

    def _background_key(self):
        L, D = self._bg_links, self._bg_data
        if not (torch.is_tensor(L) and torch.is_tensor(D)):
            return None
        return (L.data_ptr(), tuple(L.shape), L._version, D.data_ptr(), tuple(D.shape))

    def _handle(self):
        h = super()._handle()      # (a new handle resets _bg_key through _drop_handle)
        key = self._background_key()
        if key is not None and key == self._bg_key:
            return h
        L, D = self._bg_links, self._bg_data
        for name, t, dt in (("background_links", L, torch.int32), ("background_data", D, torch.float32)):
            if not torch.is_tensor(t):
                raise TypeError(f"{name} must be a tensor")
            if not t.is_cuda:
                raise RuntimeError(f"{name} is on the CPU: BackgroundGrid has no CPU fallback")
            if t.device != self.ctx.device:
                raise RuntimeError(f"{name} is on {t.device}, the grid on {self.ctx.device}")
            if t.dtype != dt:
                raise TypeError(f"{name} must be {dt}, got {t.dtype}")
            if not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
            if t.requires_grad:
                raise NotImplementedError("gradients to the background (training it) are not built")
        if L.dim() != 2 or L.shape[0] != 2 * L.shape[1] or D.dim() != 3 or D.shape[2] != 4:
            raise ValueError(f"mismatched shapes: background_links {tuple(L.shape)} [2 R, R], background_data {tuple(D.shape)} "
                             "[capacity, L, 4]")
        nl, R = _check_nlayers_reso(D.shape[1], L.shape[1])
        d = GridBackgroundDesc()
        d.nlayers, d.reso, d.capacity = nl, R, int(D.shape[0])
        d.links, d.data = L.data_ptr(), D.data_ptr()
        d.stream = self.ctx.stream().value
        check(self.ctx.lib.nerf_grid_set_background(h, C.byref(d)))
        self._bg_shape()
        self._bg_key = key
        return h

    # ---- rendering ------------------------------------------------------------------------------------------
    def _render(self, cam, rays, randomize, return_log_transmit, counters):
        """The foreground with ``background_brightness`` 0 and its ``log_transmit``, then the background pass on both, on the
        same stream. (``counters``: the instrumented foreground launch of ``count_samples``, which has no background.)"""
        if counters is not None:
            return super()._render(cam, rays, randomize, return_log_transmit, counters)
        opt = self.opt._to_c(randomize)
        fg_opt = self.opt._to_c(randomize)
        fg_opt.background_brightness = 0.0
        h = self._handle()
        lib, stream = self.ctx.lib, self.ctx.stream().value
        a, b = GridRenderArgs(), GridBackgroundArgs()
        if cam is not None:
            if isinstance(cam, NdcCamera):
                raise NotImplementedError("background layers are for unbounded scenes: svox2 never combines them with NDC, and "
                                          "an NdcCamera is refused")
            c = cam._to_c()
            n = cam.width * cam.height
        else:
            o = self._rays_arg(rays.origins, "rays.origins")
            d = self._rays_arg(rays.dirs, "rays.dirs", o.shape[0])
            n = o.shape[0]
            a.origins, a.dirs, a.n_rays = o.data_ptr(), d.data_ptr(), n
            b.origins, b.dirs, b.n_rays = o.data_ptr(), d.data_ptr(), n
        rgb = torch.empty((n, 3), device=self.ctx.device, dtype=torch.float32)
        logt = torch.empty((n,), device=self.ctx.device, dtype=torch.float32)
        a.rgb, a.log_transmit, a.counters, a.use_skip, a.stream = rgb.data_ptr(), logt.data_ptr(), 0, 1, stream
        b.rgb, b.log_transmit, b.stream = rgb.data_ptr(), logt.data_ptr(), stream
        if cam is not None:
            check(lib.nerf_grid_render_image(h, C.byref(c), C.byref(fg_opt), C.byref(a)))
            check(lib.nerf_grid_background_image(h, C.byref(c), C.byref(opt), C.byref(b)))
        else:
            check(lib.nerf_grid_render_rays(h, C.byref(fg_opt), C.byref(a)))
            check(lib.nerf_grid_background_rays(h, C.byref(opt), C.byref(b)))
        return (rgb, logt) if return_log_transmit else rgb

    # ---- thinning -------------------------------------------------------------------------------------------
    def sparsify_background(self, sigma_thresh: float = 1.0, dilate: int = 1):
        """svox2's ``sparsify_background``, in place and on the device: a texel is kept iff it has a row and, after ``dilate``
        dilations of the ``[2 R, R, L]`` volume ``sigma >= sigma_thresh`` (27-neighbourhood, clamped at the faces, no wrap
        across the seam - svox2's), any of its layers is set. ``background_links`` is rewritten in place (kept texels
        numbered in C order, the others -1) and ``background_data`` becomes a new tensor of the kept rows. The number of kept
        rows is the one value read back from the device. The foreground and its skip data are not touched. Returns that
        number."""
        sigma_thresh, dilate = float(sigma_thresh), int(dilate)
        if sigma_thresh != sigma_thresh or dilate < 0:
            raise ValueError(f"sigma_thresh = {sigma_thresh} must not be NaN, dilate = {dilate} not negative")
        self._handle()      # validates the tensors
        ctx, dev = self.ctx, self.ctx.device
        L, D = self._bg_links, self._bg_data
        R, nl = int(L.shape[1]), int(D.shape[1])
        texels = 2 * R * R
        mask = torch.empty((2, texels * nl), dtype=torch.uint8, device=dev)
        keep = torch.empty((texels,), dtype=torch.uint8, device=dev)
        offsets = torch.empty((max(1, int(ctx.lib.nerf_grid_compact_workspace(texels))),), dtype=torch.int32, device=dev)
        new_links = torch.empty_like(L)
        count = torch.zeros((1,), dtype=torch.int32, device=dev)
        a = GridBackgroundSparsifyArgs()
        a.nlayers, a.reso, a.capacity = nl, R, int(D.shape[0])
        a.links, a.data, a.sigma_thresh, a.dilate = L.data_ptr(), D.data_ptr(), sigma_thresh, dilate
        a.mask, a.keep, a.block_offsets = mask.data_ptr(), keep.data_ptr(), offsets.data_ptr()
        a.new_links, a.count, a.stream = new_links.data_ptr(), count.data_ptr(), ctx.stream().value
        check(ctx.lib.nerf_grid_background_sparsify_plan(ctx.handle, C.byref(a)))
        kept = int(count.item())      # the one readback
        new_data = torch.empty((kept, nl, 4), dtype=torch.float32, device=dev)
        t = GridBackgroundGatherArgs()
        t.nlayers, t.reso, t.capacity = nl, R, int(D.shape[0])
        t.links, t.data, t.new_links = L.data_ptr(), D.data_ptr(), new_links.data_ptr()
        t.new_capacity, t.new_data, t.stream = kept, new_data.data_ptr(), ctx.stream().value
        check(ctx.lib.nerf_grid_background_gather(ctx.handle, C.byref(t)))
        L.copy_(new_links)      # in place: an alias of background_links sees the new links
        self.background_data = new_data
        return kept

    # ---- files ----------------------------------------------------------------------------------------------
    def save(self, path: str, compress: bool = False):
        """svox2's ``.npz`` as ``SparseGrid.save`` writes it, and ``background_links`` int32 ``[2 R, R]`` (every negative link
        as -1), ``background_data`` fp32 ``[capacity, L, 4]``."""
        links = self._links.detach().cpu().numpy()
        bl = self._bg_links.detach().cpu().numpy()
        data = {
            "radius": self.radius.numpy(),
            "center": self.center.numpy(),
            "links": np.where(links < 0, np.int32(-1), links).astype(np.int32),
            "density_data": self._density.detach().cpu().numpy(),
            "sh_data": self._sh.detach().cpu().numpy().astype(np.float16),
            "basis_type": self.basis_type,
            "background_links": np.where(bl < 0, np.int32(-1), bl).astype(np.int32),
            "background_data": self._bg_data.detach().cpu().numpy().astype(np.float32),
        }
        (np.savez_compressed if compress else np.savez)(path, **data)

    @staticmethod
    def read_npz(path):
        """The arrays of an svox2 ``.npz`` WITH a background as numpy, on the host: those of ``SparseGrid.read_npz`` and
        ``background_links`` int32, ``background_data`` fp32. ``ValueError`` for a file without a background."""
        z = np.load(path)
        if "background_data" not in z.files or "background_links" not in z.files:
            raise ValueError(f"{path} holds no background layers (background_links / background_data): open it with "
                             "SparseGrid.load, or with load_grid, which picks the class")
        basis_type = int(z["basis_type"].item()) if "basis_type" in z.files else BASIS_TYPE_SH
        if basis_type != BASIS_TYPE_SH or "basis_data" in z.files:
            raise NotImplementedError("only spherical harmonics (BASIS_TYPE_SH) are built, not learned bases")
        if "data" in z.files:
            sh_data, density_data = z["data"][..., 1:], z["data"][..., :1]
        else:
            sh_data, density_data = z["sh_data"], z["density_data"]
        host = lambda a, dt: np.ascontiguousarray(np.asarray(a).astype(dt))      # noqa: E731
        bl, bd = host(z["background_links"], np.int32), host(z["background_data"], np.float32)
        if bl.ndim != 2 or bl.shape[0] != 2 * bl.shape[1] or bd.ndim != 3 or bd.shape[2] != 4:
            raise ValueError(f"background_links {bl.shape} must be [2 R, R] and background_data {bd.shape} [capacity, L, 4]")
        return {"links": host(z["links"], np.int32), "density_data": host(density_data, np.float32),
                "sh_data": host(sh_data, np.float32), "background_links": bl, "background_data": bd,
                "radius": z["radius"].tolist() if "radius" in z.files else [1.0, 1.0, 1.0],
                "center": z["center"].tolist() if "center" in z.files else [0.0, 0.0, 0.0]}

    @classmethod
    def load(cls, path: str, device: Union[torch.device, str] = "cuda"):
        """A grid from svox2's ``.npz`` with ``background_links`` / ``background_data``; ``ValueError`` naming
        ``SparseGrid.load`` for a file without them."""
        a = cls.read_npz(path)
        if torch.device(device).type != "cuda":
            raise RuntimeError(f"device {device} is not a GPU: BackgroundGrid has no CPU fallback")
        dev = get_context(device).device
        t = {k: torch.from_numpy(a[k]).to(dev) for k in ("links", "density_data", "sh_data", "background_links", "background_data")}
        return cls.from_tensors(t["links"], t["density_data"], t["sh_data"], a["radius"], a["center"],
                                background_links=t["background_links"], background_data=t["background_data"])

    # ---- what a SparseGrid has and this one does not ------------------------------------------------------------
    @classmethod
    def from_nerf(cls, *a, **k):
        raise NotImplementedError("BackgroundGrid.from_nerf: bake a SparseGrid and pass it to BackgroundGrid.from_grid")

    def _like(self, *a, **k):
        raise NotImplementedError("a BackgroundGrid is not resampled or pruned: use foreground()")


def load_grid(path: str, device: Union[torch.device, str] = "cuda"):
    """The grid of an svox2 ``.npz``: a ``BackgroundGrid`` if the file has ``background_data``, else a ``SparseGrid``."""
    with np.load(path) as z:
        has_background = "background_data" in z.files
    return (BackgroundGrid if has_background else SparseGrid).load(path, device)
