"""Occupancy-grid rendering: skip the network at samples in empty space.

An :class:`OccupancyGrid` is one bit per cell of the lattice ``density_grid`` evaluates (``reso`` nodes per axis,
``reso - 1`` cells). ``render_rays(..., occupancy=occ)`` / ``render(..., occupancy=occ)`` (and ``render_path`` through
``render_kwargs_test["occupancy"]``) evaluate the network only at samples whose cell is occupied - plus the last sample
of every ray, always - and write zeros to ``raw`` everywhere else; the semantics are stated in include/nerf_mi355x.h,
"Occupancy grid". ``train_on_batch(..., occupancy=occ)`` trains through the kept samples alone. The grid is a snapshot
of the networks it was built from: :meth:`OccupancyGrid.refresh` re-evaluates it in place every so many training steps.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import OccupancyArgs, check
from .host import NeRF, get_context
from .mesh import _axes, density_grid

__all__ = ["OccupancyGrid"]

_OUTSIDE = {"evaluate": _lib.NERF_OCC_EVALUATE, "empty": _lib.NERF_OCC_EMPTY}


class OccupancyGrid:
    """Cells of the box ``[c1, c2]`` that may hold density. Build one with :meth:`build` or :meth:`from_mask`."""

    def __init__(self, ctx, c1, c2, reso, lattices, cell_mask, threshold, dilate, outside):
        if outside not in _OUTSIDE:
            raise ValueError(f"outside {outside!r}: expected one of {sorted(_OUTSIDE)}")
        self.ctx = ctx
        self.c1, self.c2, self.reso = c1, c2, reso
        self.outside, self.threshold, self.dilate = outside, float(threshold), int(dilate)
        a, _keep = self._args(lattices, cell_mask)
        handle = C.c_void_p()
        self._handle = None
        check(ctx.lib.nerf_occupancy_create(ctx.handle, C.byref(a), C.byref(handle)))      # (synchronises the stream)
        self._handle = handle
        n = C.c_int64()
        check(ctx.lib.nerf_occupancy_cells(self._handle, None, C.byref(n), None))
        self.n_occupied = n.value

    def _args(self, lattices, cell_mask):
        a = OccupancyArgs()
        a.c1[:], a.c2[:], a.reso[:] = self.c1, self.c2, self.reso
        a.n_lattices = len(lattices)
        ptrs = (C.c_void_p * max(len(lattices), 1))(*[t.data_ptr() for t in lattices])
        a.sigma = C.cast(ptrs, C.POINTER(C.c_void_p))
        a.cell_mask = 0 if cell_mask is None else cell_mask.data_ptr()
        a.threshold, a.dilate, a.outside = self.threshold, self.dilate, _OUTSIDE[self.outside]
        a.stream = self.ctx.stream().value
        return a, ptrs

    def refresh(self, networks):
        """Re-evaluates the grid in place from the networks as they are now: ``density_grid`` of each on the grid's own
        lattice, then the cells by the grid's own ``threshold`` / ``dilate`` / ``outside`` - afterwards ``cells()`` equals
        those of a fresh :meth:`build` with the same arguments. The handle and the ``stats()`` counters survive;
        ``n_occupied`` is updated. Returns ``self``."""
        nets = [networks] if isinstance(networks, NeRF) else list(networks)
        if not nets or not all(isinstance(n, NeRF) for n in nets):
            raise TypeError("OccupancyGrid.refresh needs this package's NeRF (or a list of them)")
        if any(n.ctx is not self.ctx for n in nets):
            raise ValueError("OccupancyGrid.refresh: the networks live on another device than the grid")
        with torch.no_grad():
            lattices = [density_grid(n, self.c1, self.c2, self.reso) for n in nets]
        a, _keep = self._args(lattices, None)
        check(self.ctx.lib.nerf_occupancy_refresh(self._handle, C.byref(a)))      # (synchronises the stream)
        n = C.c_int64()
        check(self.ctx.lib.nerf_occupancy_cells(self._handle, None, C.byref(n), None))
        self.n_occupied = n.value
        return self

    def __del__(self):
        if getattr(self, "_handle", None) is not None:
            try:
                self.ctx.lib.nerf_occupancy_destroy(self._handle)
            except Exception:      # (interpreter shutdown)
                pass
            self._handle = None

    @classmethod
    def build(cls, networks, c1, c2, reso, threshold=0.0, dilate=1, outside="evaluate"):
        """The grid of one ``NeRF`` or of a list of them (the union: ``[network_fn, network_fine]`` serves both passes):
        ``density_grid`` of every network on ``reso`` nodes over ``[c1, c2]``, a cell occupied when sigma at any of its 8
        corners is ``> threshold`` (or NaN) in any network, grown by ``dilate`` cells in all 26 directions. ``outside``:
        what happens to samples outside the box, "evaluate" (the network runs) or "empty" (skipped)."""
        nets = [networks] if isinstance(networks, NeRF) else list(networks)
        if not nets or not all(isinstance(n, NeRF) for n in nets):
            raise TypeError("OccupancyGrid.build needs this package's NeRF (or a list of them)")
        if any(n.ctx is not nets[0].ctx for n in nets):
            raise ValueError("OccupancyGrid.build: the networks live on different devices")
        c1, c2, reso = _axes(c1, c2, reso)
        with torch.no_grad():
            lattices = [density_grid(n, c1, c2, reso) for n in nets]
        return cls(nets[0].ctx, c1, c2, reso, lattices, None, threshold, dilate, outside)

    @classmethod
    def from_mask(cls, mask, c1, c2, outside="evaluate"):
        """A grid with exactly the cells of ``mask`` (bool ``[X-1, Y-1, Z-1]``, tensor or array) over ``[c1, c2]``."""
        ctx = get_context(mask.device) if torch.is_tensor(mask) and mask.is_cuda else get_context()
        m = torch.as_tensor(mask).to(device=ctx.device)
        if m.dim() != 3:
            raise ValueError(f"expected a cell mask [X-1, Y-1, Z-1], got shape {tuple(m.shape)}")
        m = (m != 0).to(torch.uint8).contiguous()
        c1, c2, reso = _axes(c1, c2, [d + 1 for d in m.shape])
        return cls(ctx, c1, c2, reso, [], m, 0.0, 0, outside)

    def _handle_for(self, ctx):
        if ctx is not self.ctx:
            raise ValueError("the occupancy grid was built on another device than the networks being rendered")
        return self._handle

    def cells(self):
        """bool tensor ``[X-1, Y-1, Z-1]`` on the device: the occupied cells."""
        out = torch.empty(tuple(r - 1 for r in self.reso), device=self.ctx.device, dtype=torch.uint8)
        check(self.ctx.lib.nerf_occupancy_cells(self._handle, out.data_ptr(), None, self.ctx.stream().value))
        return out.bool()

    @property
    def occupied_fraction(self):
        n = 1
        for r in self.reso:
            n *= r - 1
        return self.n_occupied / n

    def stats(self, reset=True):
        """``(evaluated, total)``: points the network evaluated and points of all passes rendered with this grid since the
        last reset. Waits for the device."""
        ev, tot = C.c_int64(), C.c_int64()
        check(self.ctx.lib.nerf_occupancy_stats(self._handle, C.byref(ev), C.byref(tot), int(bool(reset))))
        return ev.value, tot.value
