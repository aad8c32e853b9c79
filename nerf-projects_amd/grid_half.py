"""Sparse voxel grid with half-precision colours: ``HalfGrid``, the inference-side twin of ``SparseGrid`` whose SH table
lives on the GPU in fp16, as a Plenoxels checkpoint stores it.

``HalfGrid.from_grid(grid)`` (or ``grid.to_half()``) packs the fp32 table of a ``SparseGrid`` once; ``HalfGrid.load(path)``
packs a checkpoint's fp16 table in row chunks without ever holding it in fp32. The packed table ``sh_half`` is
``torch.float16 [capacity, row_halfs]`` with 64 / 32 / 8 bytes per row at ``basis_dim`` 9 / 4 / 1 (fp32: 108 / 48 / 12); its
layout belongs to the kernels (include/nerf_mi355x.h, "Sparse voxel grid: half-precision colours") and nothing here reads
it except through ``nerf_grid_pack_half`` / ``nerf_grid_unpack_half``. ``links`` and ``density_data`` are shared with the
source grid by reference.

Rendering, sampling and saving never materialise the fp32 table. A half is widened when the kernel loads it and everything
after that is ``SparseGrid``'s fp32 arithmetic in the same order, so ``volume_render``, ``volume_render_image`` and
``sample`` return, bit for bit, what ``SparseGrid`` returns on the widened table (:meth:`HalfGrid.to_float`): a grid that came
from a checkpoint renders losslessly. Everything that reads density only - depth, ray lengths, ``accelerate``,
``compute_FDR``, ``label_components``, the floater views - takes a ``HalfGrid`` as it is. What reads or writes an fp32 SH
table - ``GridTrainer``, ``GridModule``, ``resample_grid``, ``remove_floaters`` - raises a ``TypeError`` that names
:meth:`HalfGrid.to_float`. As everywhere in this package there is no CPU or PyTorch fallback.
"""
import ctypes as C
import warnings
from dataclasses import replace
from typing import Optional, Union

import numpy as np
import torch

from . import _lib
from ._lib import GridHalfDesc, GridPackHalfArgs, check
from .grid import BASIS_TYPE_SH, SparseGrid
from .host import get_context

__all__ = ["HalfGrid", "row_halfs"]

_LANES = {None: _lib.NERF_GRID_HALF_LANES_DEFAULT, "single": _lib.NERF_GRID_HALF_LANES_SINGLE,
          "pair": _lib.NERF_GRID_HALF_LANES_PAIR}
_CHUNK_ROWS = 1 << 16      # rows converted at a time by load / save: 7 MB of fp32 at basis_dim 9


def row_halfs(basis_dim):
    """Halfs in one packed row: 32 / 16 / 4 at ``basis_dim`` 9 / 4 / 1. Needs no GPU."""
    n = _lib.load().nerf_grid_half_row_halfs(int(basis_dim))
    if n < 0:
        raise ValueError(f"basis_dim {basis_dim}: spherical harmonics of 1, 4 or 9 coefficients are built")
    return n


def _pack(ctx, sh, sh_half, row0, basis_dim, clamped):
    """Rows of fp32 ``sh [rows, 3 * basis_dim]`` into rows ``[row0, row0 + rows)`` of ``sh_half``; ``clamped`` (int64 ``[1]``
    on the device, or None) is incremented."""
    a = GridPackHalfArgs()
    a.basis_dim, a.capacity, a.row0, a.rows = basis_dim, int(sh_half.shape[0]), row0, int(sh.shape[0])
    a.sh_data, a.sh_half = sh.data_ptr(), sh_half.data_ptr()
    a.clamped = 0 if clamped is None else clamped.data_ptr()
    a.stream = ctx.stream().value
    check(ctx.lib.nerf_grid_pack_half(ctx.handle, C.byref(a)))


def _unpack(ctx, sh_half, row0, rows, basis_dim):
    """Rows ``[row0, row0 + rows)`` of ``sh_half`` widened: fp32 ``[rows, 3 * basis_dim]``."""
    out = torch.empty((rows, 3 * basis_dim), dtype=torch.float32, device=ctx.device)
    if rows:
        check(ctx.lib.nerf_grid_unpack_half(ctx.handle, sh_half[row0:].data_ptr(), rows, basis_dim, out.data_ptr(), ctx.stream()))
    return out


def _warn_clamped(clamped, who):
    n = int(clamped.item())      # the one readback of a one-off conversion
    if n:
        warnings.warn(f"{who}: {n} SH coefficient(s) beyond +-65504 were clamped to the largest half", RuntimeWarning, stacklevel=3)
    return n


class HalfGrid(SparseGrid):
    """A ``SparseGrid`` for inference whose colours are ``sh_half`` (``torch.float16 [capacity, row_halfs(basis_dim)]``, packed
    by the kernels) instead of ``sh_data``. Make one with :meth:`from_grid`, :meth:`load` or ``SparseGrid.to_half()``.

    ``lanes`` picks the render kernel's lane mapping - ``"single"`` (one coefficient per lane), ``"pair"`` (two) or ``None``
    (the faster one as measured); the results do not depend on it."""

    is_half = True

    def __init__(self, *a, **k):
        raise TypeError("a HalfGrid is made from a grid or a file: HalfGrid.from_grid(grid), grid.to_half(), HalfGrid.load(path)")

    @classmethod
    def _around(cls, links, density_data, sh_half, radius, center, basis_dim, lanes=None):
        if lanes not in _LANES:
            raise ValueError(f"lanes = {lanes!r} must be None, 'single' or 'pair'")
        g = cls.__new__(cls)
        g._init_common(list(links.shape), radius, center, BASIS_TYPE_SH, basis_dim, 0, links.device)
        g.capacity = int(density_data.shape[0])
        g._links, g._density, g._sh, g._sh_half, g._lanes = links, density_data, None, sh_half, lanes
        g._handle()      # validates
        return g

    @classmethod
    def from_tensors(cls, links, density_data, sh_half, radius, center, basis_dim=None, lanes=None):
        """A grid around existing device tensors (borrowed): ``sh_half`` is a packed table, fp16
        ``[capacity, row_halfs(basis_dim)]``, and ``basis_dim`` is required (the row length does not determine it for a
        reader that does not know the layout)."""
        if basis_dim is None:
            raise ValueError("HalfGrid.from_tensors needs basis_dim")
        links = torch.as_tensor(links)
        if links.dim() != 3:
            raise ValueError(f"links must be [X, Y, Z], got shape {tuple(links.shape)}")
        if not links.is_cuda:
            raise RuntimeError("links is on the CPU: HalfGrid has no CPU fallback (pass device tensors)")
        return cls._around(links, torch.as_tensor(density_data), torch.as_tensor(sh_half), radius, center, basis_dim, lanes)

    @classmethod
    def from_grid(cls, grid: SparseGrid, lanes: Optional[str] = None):
        """The half twin of ``grid``: ``links`` and ``density_data`` are ``grid``'s own tensors, ``sh_half`` is new,
        ``opt`` is a copy. A coefficient beyond +-65504 becomes the largest half; the count of those is read back once and
        warned about."""
        if isinstance(grid, HalfGrid):
            g = cls._around(grid._links, grid._density, grid._sh_half.clone(), grid.radius, grid.center, grid.basis_dim, lanes)
            g.opt = replace(grid.opt)
            return g
        if not isinstance(grid, SparseGrid):
            raise TypeError("HalfGrid.from_grid needs a SparseGrid")
        if grid.use_background:
            raise NotImplementedError("HalfGrid.from_grid: half-precision colours with background layers are not built: pass "
                                      "grid.foreground()")
        grid._handle()      # validates the tensors
        ctx = grid.ctx
        sh_half = torch.empty((grid.capacity, row_halfs(grid.basis_dim)), dtype=torch.float16, device=ctx.device)
        clamped = torch.zeros(1, dtype=torch.int64, device=ctx.device)
        _pack(ctx, grid.sh_data, sh_half, 0, grid.basis_dim, clamped)
        _warn_clamped(clamped, "HalfGrid.from_grid")
        g = cls._around(grid.links, grid.density_data, sh_half, grid.radius, grid.center, grid.basis_dim, lanes)
        g.opt = replace(grid.opt)
        return g

    # ---- the borrowed tensors -------------------------------------------------------------------------------
    @property
    def sh_half(self):
        return self._sh_half

    @sh_half.setter
    def sh_half(self, t):
        self._drop_handle()
        self._sh_half = t

    @property
    def sh_data(self):
        raise TypeError("a HalfGrid holds no fp32 sh_data (sh_half is its packed fp16 table): to_float() widens it")

    @sh_data.setter
    def sh_data(self, t):
        raise TypeError("a HalfGrid holds no fp32 sh_data: update_sh(sh_data) repacks new coefficients into sh_half")

    @property
    def data_dim(self):
        return 3 * self.basis_dim + 1

    @property
    def sh_bytes(self):
        """Bytes of the packed colour table."""
        return self._sh_half.numel() * 2

    def _key(self):
        tensors = (self._links, self._density, self._sh_half)
        if not all(torch.is_tensor(t) for t in tensors):
            return None
        return tuple((t.data_ptr(), tuple(t.shape)) for t in tensors) + (self._links._version, self._lanes)

    def _handle(self):
        key = self._key()
        if self._handle_ptr is not None and key == self._handle_key:
            return self._handle_ptr
        self._drop_handle()
        L, D, S = self._links, self._density, self._sh_half
        for name, t, dt in (("links", L, torch.int32), ("density_data", D, torch.float32), ("sh_half", S, torch.float16)):
            if not torch.is_tensor(t):
                raise TypeError(f"{name} must be a tensor")
            if not t.is_cuda:
                raise RuntimeError(f"{name} is on the CPU: HalfGrid has no CPU fallback")
            if t.device != self.ctx.device:
                raise RuntimeError(f"{name} is on {t.device}, the grid on {self.ctx.device}")
            if t.dtype != dt:
                raise TypeError(f"{name} must be {dt}, got {t.dtype}")
            if not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
            if t.requires_grad:
                raise NotImplementedError("gradients through a HalfGrid are not built: train the SparseGrid of to_float()")
        cap, rh = int(D.shape[0]), row_halfs(self.basis_dim)
        if L.dim() != 3 or D.dim() != 2 or D.shape[1] != 1 or S.dim() != 2 or tuple(S.shape) != (cap, rh):
            raise ValueError(f"mismatched shapes: links {tuple(L.shape)} [X, Y, Z], density_data {tuple(D.shape)} [capacity, 1], "
                             f"sh_half {tuple(S.shape)} [capacity, {rh}]")
        d = GridHalfDesc()
        d.reso[:] = list(L.shape)
        d.basis_dim = self.basis_dim
        d.radius[:] = self.radius.tolist()
        d.center[:] = self.center.tolist()
        d.capacity = cap
        d.links, d.density_data, d.sh_half = L.data_ptr(), D.data_ptr(), S.data_ptr()
        d.lanes = _LANES[self._lanes]
        d.stream = self.ctx.stream().value
        h = C.c_void_p()
        check(self.ctx.lib.nerf_grid_create_half(self.ctx.handle, C.byref(d), C.byref(h)))
        self.capacity = cap
        self._handle_ptr, self._handle_key = h, key
        return h

    # ---- conversions ------------------------------------------------------------------------------------------
    def to_float(self) -> SparseGrid:
        """A ``SparseGrid`` on the exactly widened table (new), sharing ``links`` and ``density_data``, with a copy of ``opt``.
        It renders what this grid renders, bit for bit."""
        sh = _unpack(self.ctx, self._sh_half, 0, self.capacity, self.basis_dim)
        g = SparseGrid.from_tensors(self._links, self._density, sh, self.radius, self.center, basis_dim=self.basis_dim)
        g.opt = replace(self.opt)
        return g

    def to_half(self, lanes: Optional[str] = None):
        return HalfGrid.from_grid(self, lanes=lanes)

    def update_sh(self, sh_data: torch.Tensor):
        """Repack fp32 ``sh_data [capacity, 3 * basis_dim]`` into the existing table (a preview of a grid in training): the
        next render reads the new colours; handle, skip data and everything else stay."""
        if not torch.is_tensor(sh_data):
            raise TypeError("sh_data must be a tensor")
        if not sh_data.is_cuda or sh_data.device != self.ctx.device:
            raise RuntimeError(f"sh_data is on {sh_data.device}, the grid on {self.ctx.device}: HalfGrid has no CPU fallback")
        if sh_data.dtype != torch.float32 or tuple(sh_data.shape) != (self.capacity, 3 * self.basis_dim):
            raise ValueError(f"sh_data must be float32 [{self.capacity}, {3 * self.basis_dim}], got {sh_data.dtype} "
                             f"{tuple(sh_data.shape)}")
        self._handle()
        clamped = torch.zeros(1, dtype=torch.int64, device=self.ctx.device)
        _pack(self.ctx, sh_data.detach().contiguous(), self._sh_half, 0, self.basis_dim, clamped)
        _warn_clamped(clamped, "HalfGrid.update_sh")

    # ---- files ------------------------------------------------------------------------------------------------
    def save(self, path: str, compress: bool = False):
        """svox2's ``.npz`` as ``SparseGrid.save`` writes it, ``sh_data`` being the halves as they are: lossless, and readable
        by ``SparseGrid.load``, by :meth:`load` and by the reference. The table is widened and narrowed again (both exact)
        a chunk of rows at a time."""
        links = self._links.detach().cpu().numpy()
        sh = np.empty((self.capacity, 3 * self.basis_dim), dtype=np.float16)
        for r0 in range(0, self.capacity, _CHUNK_ROWS):
            rows = min(_CHUNK_ROWS, self.capacity - r0)
            sh[r0:r0 + rows] = _unpack(self.ctx, self._sh_half, r0, rows, self.basis_dim).to(torch.float16).cpu().numpy()
        data = {
            "radius": self.radius.numpy(),
            "center": self.center.numpy(),
            "links": np.where(links < 0, np.int32(-1), links).astype(np.int32),
            "density_data": self._density.detach().cpu().numpy(),
            "sh_data": sh,
            "basis_type": self.basis_type,
        }
        (np.savez_compressed if compress else np.savez)(path, **data)

    @classmethod
    def load(cls, path: str, device: Union[torch.device, str] = "cuda", lanes: Optional[str] = None):
        """A grid from svox2's ``.npz``. The file's table (fp16 in a checkpoint) goes to the GPU a chunk of rows at a time and
        is packed there: no fp32 copy of the whole table exists on either side. Refuses what ``SparseGrid.load`` refuses."""
        z = np.load(path)
        if "background_data" in z.files:
            raise NotImplementedError("background MSI layers are not built")
        basis_type = int(z["basis_type"].item()) if "basis_type" in z.files else BASIS_TYPE_SH
        if basis_type != BASIS_TYPE_SH or "basis_data" in z.files:
            raise NotImplementedError("only spherical harmonics (BASIS_TYPE_SH) are built, not learned bases")
        if torch.device(device).type != "cuda":
            raise RuntimeError(f"device {device} is not a GPU: HalfGrid has no CPU fallback")
        if "data" in z.files:      # the old layout: one array, density first
            sh, density = z["data"][..., 1:], z["data"][..., :1]
        else:
            sh, density = z["sh_data"], z["density_data"]
        if sh.ndim != 2 or sh.shape[1] % 3 or sh.shape[1] // 3 not in (1, 4, 9):
            raise ValueError(f"sh_data must be [capacity, 3 * basis_dim] with basis_dim 1, 4 or 9, got shape {sh.shape}")
        basis_dim, cap = sh.shape[1] // 3, sh.shape[0]
        ctx = get_context(device)
        dev = ctx.device
        sh_half = torch.empty((cap, row_halfs(basis_dim)), dtype=torch.float16, device=dev)
        clamped = torch.zeros(1, dtype=torch.int64, device=dev)
        for r0 in range(0, cap, _CHUNK_ROWS):
            chunk = torch.from_numpy(np.ascontiguousarray(sh[r0:r0 + _CHUNK_ROWS])).to(dev).to(torch.float32)
            _pack(ctx, chunk, sh_half, r0, basis_dim, clamped)
        _warn_clamped(clamped, "HalfGrid.load")
        links = torch.from_numpy(np.ascontiguousarray(z["links"].astype(np.int32))).to(dev)
        density = torch.from_numpy(np.ascontiguousarray(np.asarray(density).astype(np.float32))).to(dev)
        radius = z["radius"].tolist() if "radius" in z.files else [1.0, 1.0, 1.0]
        center = z["center"].tolist() if "center" in z.files else [0.0, 0.0, 0.0]
        return cls._around(links, density, sh_half, radius, center, basis_dim, lanes)

    # ---- what a SparseGrid has and this one does not ------------------------------------------------------------
    @classmethod
    def from_nerf(cls, *a, **k):
        raise NotImplementedError("HalfGrid.from_nerf: bake a SparseGrid and call to_half() on it")

    @staticmethod
    def read_npz(path):
        raise NotImplementedError("HalfGrid.read_npz: SparseGrid.read_npz reads the arrays of a file (widened to fp32)")

    def _like(self, *a, **k):
        raise TypeError("a HalfGrid has no fp32 SH table to copy rows of: use to_float()")
