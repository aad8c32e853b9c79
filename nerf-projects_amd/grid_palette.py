"""Sparse voxel grid with palette-quantised colours: ``PaletteGrid``, the inference-side twin of ``SparseGrid`` whose colours
are one ``uint16`` palette index per node and SH basis function - PlenOctree's ``octree/compression.py`` on this project's grid.

``PaletteGrid.from_grid(grid, bits=16, retain=0, sigma_thresh=None)`` (or ``grid.to_palette(...)``) quantises, for every basis
function ``k >= retain`` on its own, the RGB triples ``(sh[:, k], sh[:, B + k], sh[:, 2 B + k])`` of all nodes to ``2^bits`` fp16
colours with :func:`quantize_median_cut`; the first ``retain`` functions stay as fp16 triples. A node then costs
``2 (B - retain) + 6 retain`` bytes of colour (18 at ``basis_dim`` 9: 0.17 of fp32, 0.28 of ``HalfGrid``'s packed row); the
palettes together are ``6 (B - retain) 2^bits`` bytes (3.5 MB at 9 x 65 536). ``links`` and ``density_data`` are shared with
the source grid by reference unless ``sigma_thresh`` is given.

``sigma_thresh = x`` leaves the rows with ``density <= x`` out of the median cut and gives them density 0, index 0 and zero
retained values, literally as the reference does. Colours are interpolated independently of density, so such a row's colour -
entry 0 of every palette - enters the trilinear blend of its kept neighbours' samples: the render changes near the surface
of what was dropped, not only inside it. The default ``None`` drops nothing.

Rendering and sampling never materialise an fp32 table. A lane loads its node's index and then its component of that palette
entry (or the retained half), widens it, and everything after that is ``SparseGrid``'s fp32 arithmetic in the same order, so
``volume_render``, ``volume_render_image`` and ``sample`` return, bit for bit, what ``SparseGrid`` returns on the dequantised
table (:meth:`PaletteGrid.to_float`), with and without :meth:`accelerate`. What reads density only - depth, ray lengths,
``compute_FDR``, ``label_components``, the floater views - takes a ``PaletteGrid`` as it is. ``GridTrainer``, ``GridModule``,
``resample_grid`` and ``remove_floaters`` raise a ``TypeError`` that names :meth:`PaletteGrid.to_float`. As everywhere in this
package there is no CPU or PyTorch fallback for the kernels; the one-off table conversions around them (gathering a
function's triples, transposing to the file's layout, dequantising for ``to_float``) are torch indexing on the device.

The file is an ``.npz`` with ``links``, ``density_data``, ``radius``, ``center``, ``basis_type`` as ``SparseGrid.save`` writes
them and compression.py's names and shapes for the rest: ``quant_colors [B - retain, 2^bits, 3]`` fp16, ``quant_map
[B - retain, capacity]`` uint16, ``data_retained [retain, capacity, 3]`` fp16.
"""
import ctypes as C
from dataclasses import replace
from typing import Optional, Union

import numpy as np
import torch

from ._lib import GridMedianCutArgs, GridPaletteDesc, check
from .grid import BASIS_TYPE_SH, SparseGrid
from .host import get_context

__all__ = ["PaletteGrid", "quantize_median_cut"]


def quantize_median_cut(colors: torch.Tensor, bits: int):
    """Balanced median cut of order ``bits`` (include/nerf_mi355x.h, "Sparse voxel grid: palette-quantised colours") of
    ``colors`` fp32 ``[M, 3]`` on the GPU: ``(palette, ids)`` with ``palette`` fp16 ``[2^bits, 3]`` and ``ids`` uint16 ``[M]``,
    both on the device. ``ValueError`` if a colour is not finite. Only the count of those comes back to the host."""
    if not torch.is_tensor(colors):
        raise TypeError("colors must be a tensor")
    if not colors.is_cuda:
        raise RuntimeError("colors is on the CPU: quantize_median_cut has no CPU fallback")
    if colors.dtype != torch.float32 or colors.dim() != 2 or colors.shape[1] != 3:
        raise ValueError(f"colors must be float32 [M, 3], got {colors.dtype} {tuple(colors.shape)}")
    bits = int(bits)
    if not 1 <= bits <= 16:
        raise ValueError(f"bits = {bits} must be in [1, 16]")
    ctx = get_context(colors.device)
    colors = colors.detach().contiguous()
    m = int(colors.shape[0])
    nbytes = ctx.lib.nerf_grid_median_cut_workspace(m, bits)
    if nbytes < 0:
        check(int(nbytes))
    workspace = torch.empty(int(nbytes), dtype=torch.uint8, device=ctx.device)
    ids = torch.empty(m, dtype=torch.uint16, device=ctx.device)
    palette = torch.empty((1 << bits, 3), dtype=torch.float16, device=ctx.device)
    nonfinite = C.c_int64(0)
    a = GridMedianCutArgs()
    a.m, a.bits = m, bits
    a.colors, a.ids, a.palette = colors.data_ptr(), ids.data_ptr(), palette.data_ptr()
    a.workspace, a.workspace_bytes = workspace.data_ptr(), int(nbytes)
    a.nonfinite = C.pointer(nonfinite)
    a.stream = ctx.stream().value
    rc = ctx.lib.nerf_grid_quantize_median_cut(ctx.handle, C.byref(a))
    if nonfinite.value:
        raise ValueError(f"quantize_median_cut: {nonfinite.value} of the {m} colours have a NaN or an infinity")
    check(rc)
    return palette, ids


def _u16(t):
    """uint16 device tensors are moved and indexed through their int16 view (the same bits)."""
    return t.view(torch.int16)


class PaletteGrid(SparseGrid):
    """A ``SparseGrid`` for inference whose colours are ``quant_map`` (uint16 ``[capacity, basis_dim - retain]``, node-major),
    ``quant_colors`` (fp16 ``[basis_dim - retain, 2^bits, 3]``) and ``sh_retained`` (fp16 ``[capacity, retain, 3]``) instead of
    ``sh_data``. Make one with :meth:`from_grid`, :meth:`load` or ``SparseGrid.to_palette()``."""

    is_palette = True

    def __init__(self, *a, **k):
        raise TypeError("a PaletteGrid is made from a grid or a file: PaletteGrid.from_grid(grid), grid.to_palette(), "
                        "PaletteGrid.load(path)")

    @classmethod
    def from_tensors(cls, links, density_data, quant_map, quant_colors, sh_retained, radius, center, basis_dim=None,
                     bits=None):
        """A grid around existing device tensors (borrowed), in the device layouts of the class docstring. ``basis_dim`` and
        ``bits`` default to what the shapes say."""
        links = torch.as_tensor(links)
        if links.dim() != 3:
            raise ValueError(f"links must be [X, Y, Z], got shape {tuple(links.shape)}")
        if not links.is_cuda:
            raise RuntimeError("links is on the CPU: PaletteGrid has no CPU fallback (pass device tensors)")
        g = cls.__new__(cls)
        if quant_map.dim() != 2 or quant_colors.dim() != 3 or sh_retained.dim() != 3:
            raise ValueError("quant_map must be [capacity, Q], quant_colors [Q, 2^bits, 3], sh_retained [capacity, retain, 3]")
        bd = int(quant_map.shape[1] + sh_retained.shape[1]) if basis_dim is None else int(basis_dim)
        g._init_common(list(links.shape), radius, center, BASIS_TYPE_SH, bd, 0, links.device)
        g.capacity = int(density_data.shape[0])
        g.retain = int(sh_retained.shape[1])
        entries = int(quant_colors.shape[1])
        g.bits = max(1, entries.bit_length() - 1) if bits is None else int(bits)
        g._links, g._density, g._sh = links, density_data, None
        g._map, g._colors, g._retained = quant_map, quant_colors, sh_retained
        g._handle()      # validates
        return g

    @classmethod
    def from_grid(cls, grid: SparseGrid, bits: int = 16, retain: int = 0, sigma_thresh: Optional[float] = None):
        """The palette twin of ``grid`` (a ``SparseGrid``; a ``HalfGrid`` is widened first): see the module docstring. ``opt`` is
        a copy. A retained coefficient beyond +-65504 becomes the largest half."""
        if isinstance(grid, PaletteGrid):
            raise TypeError("PaletteGrid.from_grid: the grid is quantised already; requantise its to_float()")
        if not isinstance(grid, SparseGrid):
            raise TypeError("PaletteGrid.from_grid needs a SparseGrid")
        if grid.use_background:
            raise NotImplementedError("PaletteGrid.from_grid: a palette on background layers is not built: pass grid.foreground()")
        if getattr(grid, "is_half", False):
            grid = grid.to_float()
        bits, retain = int(bits), int(retain)
        B = grid.basis_dim
        if not 1 <= bits <= 16:
            raise ValueError(f"bits = {bits} must be in [1, 16]")
        if not 0 <= retain <= B:
            raise ValueError(f"retain = {retain} must be in [0, basis_dim = {B}]")
        grid._handle()      # validates the tensors
        dev = grid.ctx.device
        sh, density, cap = grid.sh_data, grid.density_data, grid.capacity
        kept = None
        if sigma_thresh is not None:
            x = float(sigma_thresh)
            if x != x:
                raise ValueError("sigma_thresh must not be NaN")
            keep = density[:, 0] > x
            kept = keep.nonzero().flatten()
            density = torch.where(keep[:, None], density, torch.zeros_like(density))
        triple = lambda k: torch.stack((sh[:, k], sh[:, B + k], sh[:, 2 * B + k]), dim=1)      # noqa: E731
        retained = torch.zeros((cap, retain, 3), dtype=torch.float16, device=dev)
        for k in range(retain):
            t = triple(k).clamp(-65504.0, 65504.0).to(torch.float16)
            if kept is None:
                retained[:, k] = t
            else:
                retained[kept, k] = t[kept]
        qmap = torch.zeros((cap, B - retain), dtype=torch.int16, device=dev)
        colors = torch.zeros((B - retain, 1 << bits, 3), dtype=torch.float16, device=dev)
        for q in range(B - retain):
            t = triple(retain + q)
            palette, ids = quantize_median_cut(t if kept is None else t[kept].contiguous(), bits)
            colors[q] = palette
            if kept is None:
                qmap[:, q] = _u16(ids)
            else:
                qmap[kept, q] = _u16(ids)
        g = cls.from_tensors(grid.links, density, qmap.view(torch.uint16), colors, retained, grid.radius, grid.center,
                             basis_dim=B, bits=bits)
        g.opt = replace(grid.opt)
        return g

    # ---- the borrowed tensors -------------------------------------------------------------------------------
    quant_map = property(lambda self: self._map)
    quant_colors = property(lambda self: self._colors)
    sh_retained = property(lambda self: self._retained)

    @property
    def sh_data(self):
        raise TypeError("a PaletteGrid holds no fp32 sh_data (quant_map, quant_colors and sh_retained are its colours): "
                        "to_float() dequantises them")

    @sh_data.setter
    def sh_data(self, t):
        raise TypeError("a PaletteGrid holds no fp32 sh_data: quantise the new table with PaletteGrid.from_grid")

    @property
    def data_dim(self):
        return 3 * self.basis_dim + 1

    @property
    def sh_bytes(self):
        """Bytes of the colour tables: indices, palettes and retained halves."""
        return 2 * (self._map.numel() + self._colors.numel() + self._retained.numel())

    @property
    def bytes_resident(self):
        """Bytes this grid keeps on the device: ``links``, ``density_data`` and the colour tables (skip data of
        :meth:`accelerate`, one byte per node, not counted)."""
        return self._links.numel() * 4 + self._density.numel() * 4 + self.sh_bytes

    def _key(self):
        tensors = (self._links, self._density, self._map, self._colors, self._retained)
        if not all(torch.is_tensor(t) for t in tensors):
            return None
        return tuple((t.data_ptr(), tuple(t.shape)) for t in tensors) + (self._links._version, self._map._version, self.bits)

    def _handle(self):
        key = self._key()
        if self._handle_ptr is not None and key == self._handle_key:
            return self._handle_ptr
        self._drop_handle()
        L, D, M, P, R = self._links, self._density, self._map, self._colors, self._retained
        for name, t, dt in (("links", L, torch.int32), ("density_data", D, torch.float32), ("quant_map", M, torch.uint16),
                            ("quant_colors", P, torch.float16), ("sh_retained", R, torch.float16)):
            if not torch.is_tensor(t):
                raise TypeError(f"{name} must be a tensor")
            if not t.is_cuda:
                raise RuntimeError(f"{name} is on the CPU: PaletteGrid has no CPU fallback")
            if t.device != self.ctx.device:
                raise RuntimeError(f"{name} is on {t.device}, the grid on {self.ctx.device}")
            if t.dtype != dt:
                raise TypeError(f"{name} must be {dt}, got {t.dtype}")
            if not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
            if t.requires_grad:
                raise NotImplementedError("gradients through a PaletteGrid are not built: train the SparseGrid of to_float()")
        cap, B, retain, bits = int(D.shape[0]), self.basis_dim, self.retain, self.bits
        if not 1 <= bits <= 16 or not 0 <= retain <= B:
            raise ValueError(f"bits = {bits} must be in [1, 16], retain = {retain} in [0, {B}]")
        if (L.dim() != 3 or D.dim() != 2 or D.shape[1] != 1 or tuple(M.shape) != (cap, B - retain)
                or tuple(P.shape) != (B - retain, 1 << bits, 3) or tuple(R.shape) != (cap, retain, 3)):
            raise ValueError(f"mismatched shapes: links {tuple(L.shape)} [X, Y, Z], density_data {tuple(D.shape)} [capacity, 1], "
                             f"quant_map {tuple(M.shape)} [capacity, {B - retain}], quant_colors {tuple(P.shape)} "
                             f"[{B - retain}, {1 << bits}, 3], sh_retained {tuple(R.shape)} [capacity, {retain}, 3]")
        d = GridPaletteDesc()
        d.reso[:] = list(L.shape)
        d.basis_dim, d.bits, d.retain = B, bits, retain
        d.radius[:] = self.radius.tolist()
        d.center[:] = self.center.tolist()
        d.capacity = cap
        d.links, d.density_data = L.data_ptr(), D.data_ptr()
        d.quant_map, d.quant_colors, d.data_retained = M.data_ptr(), P.data_ptr(), R.data_ptr()
        d.stream = self.ctx.stream().value
        h = C.c_void_p()
        check(self.ctx.lib.nerf_grid_create_palette(self.ctx.handle, C.byref(d), C.byref(h)))
        self.capacity = cap
        self._handle_ptr, self._handle_key = h, key
        return h

    # ---- conversions ------------------------------------------------------------------------------------------
    def _dequantised(self, dtype):
        """``[capacity, 3 * basis_dim]`` in ``dtype``: column ``c * B + k`` is the half the kernels read for (c, k)."""
        B, retain = self.basis_dim, self.retain
        out = torch.empty((self.capacity, 3, B), dtype=dtype, device=self.ctx.device)
        if retain:
            out[:, :, :retain] = self._retained.permute(0, 2, 1).to(dtype)
        for q in range(B - retain):
            idx = _u16(self._map[:, q]).to(torch.int64) & 0xFFFF
            out[:, :, retain + q] = self._colors[q][idx].to(dtype)
        return out.view(self.capacity, 3 * B)

    def to_float(self) -> SparseGrid:
        """The dequantised ``SparseGrid`` (a new fp32 table), sharing ``links`` and ``density_data``, with a copy of ``opt``.
        It renders what this grid renders, bit for bit."""
        g = SparseGrid.from_tensors(self._links, self._density, self._dequantised(torch.float32), self.radius, self.center,
                                    basis_dim=self.basis_dim)
        g.opt = replace(self.opt)
        return g

    def to_half(self, lanes: Optional[str] = None):
        """The dequantised ``HalfGrid``: exact, every value being a half already."""
        from .grid_half import HalfGrid
        return HalfGrid.from_grid(self.to_float(), lanes=lanes)

    def to_palette(self, *a, **k):
        raise TypeError("the grid is quantised already: requantise its to_float()")

    # ---- files ------------------------------------------------------------------------------------------------
    def save(self, path: str, compress: bool = False):
        """The ``.npz`` of the module docstring; negative links are written as -1 as ``SparseGrid.save`` does."""
        links = self._links.detach().cpu().numpy()
        data = {
            "radius": self.radius.numpy(),
            "center": self.center.numpy(),
            "links": np.where(links < 0, np.int32(-1), links).astype(np.int32),
            "density_data": self._density.detach().cpu().numpy(),
            "quant_colors": self._colors.cpu().numpy(),
            "quant_map": np.ascontiguousarray(_u16(self._map).cpu().numpy().view(np.uint16).T),
            "data_retained": np.ascontiguousarray(self._retained.cpu().numpy().transpose(1, 0, 2)),
            "basis_type": self.basis_type,
        }
        (np.savez_compressed if compress else np.savez)(path, **data)

    @classmethod
    def load(cls, path: str, device: Union[torch.device, str] = "cuda"):
        """A grid from the ``.npz`` :meth:`save` writes."""
        z = np.load(path)
        for name in ("links", "density_data", "quant_colors", "quant_map", "data_retained"):
            if name not in z.files:
                raise ValueError(f"{path} has no {name}: not a palette grid (SparseGrid.load / load_grid open svox2's .npz)")
        basis_type = int(z["basis_type"].item()) if "basis_type" in z.files else BASIS_TYPE_SH
        if basis_type != BASIS_TYPE_SH:
            raise NotImplementedError("only spherical harmonics (BASIS_TYPE_SH) are built, not learned bases")
        if torch.device(device).type != "cuda":
            raise RuntimeError(f"device {device} is not a GPU: PaletteGrid has no CPU fallback")
        colors, qmap, retained = z["quant_colors"], z["quant_map"], z["data_retained"]
        if (colors.dtype != np.float16 or qmap.dtype != np.uint16 or retained.dtype != np.float16 or colors.ndim != 3
                or colors.shape[2] != 3 or qmap.ndim != 2 or retained.ndim != 3 or retained.shape[2] != 3
                or qmap.shape[0] != colors.shape[0] or colors.shape[1] & (colors.shape[1] - 1) or not 2 <= colors.shape[1] <= 65536):
            raise ValueError(f"quant_colors {colors.dtype} {colors.shape} must be float16 [Q, 2^bits, 3], quant_map {qmap.dtype} "
                             f"{qmap.shape} uint16 [Q, capacity], data_retained {retained.dtype} {retained.shape} float16 "
                             "[retain, capacity, 3]")
        dev = get_context(device).device
        cap = int(z["density_data"].shape[0])
        host = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
        dmap = host(qmap.T.view(np.int16)).view(torch.uint16).reshape(cap, qmap.shape[0])
        dret = host(retained.transpose(1, 0, 2)).reshape(cap, retained.shape[0], 3)
        radius = z["radius"].tolist() if "radius" in z.files else [1.0, 1.0, 1.0]
        center = z["center"].tolist() if "center" in z.files else [0.0, 0.0, 0.0]
        return cls.from_tensors(host(z["links"].astype(np.int32)), host(z["density_data"].astype(np.float32)), dmap,
                                host(colors), dret, radius, center)

    # ---- what a SparseGrid has and this one does not ------------------------------------------------------------
    @classmethod
    def from_nerf(cls, *a, **k):
        raise NotImplementedError("PaletteGrid.from_nerf: bake a SparseGrid and call to_palette() on it")

    @staticmethod
    def read_npz(path):
        raise NotImplementedError("PaletteGrid.read_npz: SparseGrid.read_npz reads the arrays of svox2's file")

    def _like(self, *a, **k):
        raise TypeError("a PaletteGrid has no fp32 SH table to copy rows of: use to_float()")
