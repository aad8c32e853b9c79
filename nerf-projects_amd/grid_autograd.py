"""``loss.backward()`` through a sparse voxel grid: ``GridModule(grid)`` is a ``torch.nn.Module`` whose parameters are the
grid's own ``density_data`` and ``sh_data``, and whose ``volume_render``, ``volume_render_image``, ``sample``,
``volume_render_depth`` and ``volume_render_depth_image`` are differentiable with respect to them - any loss, any torch
optimiser::

    m = GridModule(grid)
    adam = torch.optim.Adam(m.parameters(), lr=1e-2)
    rgb = m.volume_render(rays); loss = anything(rgb); loss.backward(); adam.step()
    depth, log_t = m.volume_render_depth(rays, return_log_transmit=True)      # depth supervision, silhouettes, T (1 - T), ...

It is the counterpart of svox2's ``SparseGrid`` as an ``nn.Module`` (``volume_render`` / ``sample`` under autograd), beside
``SparseGrid`` and not on it: a ``SparseGrid`` itself still refuses tensors that require gradients. Everything runs in the HIP
kernels of csrc/grid_autograd_kernels.hip and csrc/grid_depth_autograd_kernels.hip; the semantics are stated in
include/nerf_mi355x.h, "Sparse voxel grid: gradients for autograd" and "Sparse voxel grid: gradients of depth and
log_transmit for autograd". The forward keeps 24 bytes per ray (the tape; 8 for a depth) for the backward; the backward
marches every ray once. The expected depth and ``log_transmit`` depend on ``density_data`` alone: ``sh_data`` gets no
gradient from them.
The regularisers of the Plenoxels objective are values too: ``tv()`` and ``tv_color()`` (svox2's, 0-dim, deterministic bits,
differentiable in ``density_data`` / ``sh_data`` respectively, over every cell or over a tensor of ``cells``) and
``sparsity_loss(rays)`` (per ray, differentiable in ``density_data``), in the kernels of csrc/grid_regularisers_kernels.hip
(include/nerf_mi355x.h, "Sparse voxel grid: regularisers as values"); the beta term is a function of ``log_transmit``::

    loss = mse + l_tv * m.tv() + l_tv_sh * m.tv_color() + l_s * m.sparsity_loss(rays).sum()

Not built: gradients with respect to rays, points or the camera, of the threshold depth (piecewise constant) or the ray
length, double backward, sparse gradient tensors.
"""
import ctypes as C
from dataclasses import replace

import torch
from torch.autograd.function import once_differentiable

from ._lib import (NERF_GRID_DEPTH_EXPECTED, NERF_GRID_TV_DENSITY, NERF_GRID_TV_SH, GridDepthBackwardArgs, GridDepthTapedArgs,
                   GridRenderBackwardArgs, GridRenderTapedArgs, GridSampleBackwardArgs, GridSparsityArgs, GridTvValueArgs, check)
from .grid import Camera, Rays, SparseGrid, _refuse_half

__all__ = ["GridModule"]


def _points_arg(t, name, device, n=None):
    """``t`` as a contiguous fp32 ``[N, 3]`` tensor on ``device``, refused in ``SparseGrid``'s vocabulary."""
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on the CPU: GridModule has no CPU fallback")
    if t.requires_grad:
        raise NotImplementedError(f"{name} requires a gradient: gradients with respect to rays and points are not built")
    if t.dim() != 2 or t.shape[1] != 3 or (n is not None and t.shape[0] != n):
        raise ValueError(f"{name} must be [N, 3], got {tuple(t.shape)}")
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def _zeros_like_or_none(t, wanted):
    return torch.zeros_like(t, memory_format=torch.contiguous_format) if wanted else None


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _same_tables(module, density, sh=None):
    """The kernels read the tables through the grid's handle: they must still be the tensors autograd saved."""
    g = module.grid
    if g.density_data.data_ptr() != density.data_ptr() or (sh is not None and g.sh_data.data_ptr() != sh.data_ptr()):
        raise RuntimeError("the grid's tables were replaced between forward and backward: run the forward again after rebind()")
    return g._handle()


class _VolumeRender(torch.autograd.Function):
    @staticmethod
    def forward(ctx, density, sh, module, o, d, want_log_transmit=False):
        g = module.grid
        opt = replace(g.opt)
        h = g._handle()
        n = o.shape[0]
        rgb = torch.empty((n, 3), device=o.device, dtype=torch.float32)
        logt = torch.empty((n if want_log_transmit else 0,), device=o.device, dtype=torch.float32)
        tape = torch.empty((n, 3), device=o.device, dtype=torch.float64)
        a = GridRenderTapedArgs()
        a.origins, a.dirs, a.n_rays = o.data_ptr(), d.data_ptr(), n
        a.rgb_out, a.log_transmit, a.tape = rgb.data_ptr(), logt.data_ptr() if want_log_transmit else 0, tape.data_ptr()
        a.use_skip = 1
        a.stream = g.ctx.stream().value
        check(g.ctx.lib.nerf_grid_render_rays_taped(h, C.byref(opt._to_c()), C.byref(a)))
        ctx.save_for_backward(density, sh, o, d, tape)      # the parameters too: torch refuses a backward after an in-place step
        ctx.module, ctx.opt, ctx.want_log_transmit = module, opt, want_log_transmit
        ctx.set_materialize_grads(False)      # an output the loss does not use arrives as None: its launch is not issued
        if not want_log_transmit:
            ctx.mark_non_differentiable(logt)
        return rgb, logt

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_rgb, grad_logt):
        density, sh, o, d, tape = ctx.saved_tensors
        g = ctx.module.grid
        h = _same_tables(ctx.module, density, sh)
        gd = _zeros_like_or_none(density, ctx.needs_input_grad[0])
        gs = _zeros_like_or_none(sh, ctx.needs_input_grad[1])
        if grad_rgb is not None:
            grad_rgb = grad_rgb.to(dtype=torch.float32).contiguous()      # (rgb.sum().backward() hands in a stride-0 expansion)
            a = GridRenderBackwardArgs()
            a.origins, a.dirs, a.n_rays = o.data_ptr(), d.data_ptr(), o.shape[0]
            a.grad_rgb, a.tape = grad_rgb.data_ptr(), tape.data_ptr()
            a.grad_density, a.grad_sh, a.mask = _ptr(gd), _ptr(gs), 0
            a.use_skip = 1
            a.stream = g.ctx.stream().value
            check(g.ctx.lib.nerf_grid_render_backward(h, C.byref(ctx.opt._to_c()), C.byref(a)))
        if grad_logt is not None and ctx.want_log_transmit and gd is not None:
            _depth_backward(g, h, ctx.opt, o, d, None, grad_logt, None, gd)      # log_transmit depends on density_data alone
        return gd, gs, None, None, None, None


def _depth_backward(g, h, opt, o, d, grad_depth, grad_logt, tape, gd):
    """One nerf_grid_depth_backward launch that takes both cotangents (either may be None) and adds to ``gd``."""
    if o.shape[0] == 0:      # (an empty tensor has no address to hand over)
        return
    grad_depth = None if grad_depth is None else grad_depth.to(dtype=torch.float32).contiguous()
    grad_logt = None if grad_logt is None else grad_logt.to(dtype=torch.float32).contiguous()
    a = GridDepthBackwardArgs()
    a.origins, a.dirs, a.n_rays = o.data_ptr(), d.data_ptr(), o.shape[0]
    a.grad_depth, a.grad_log_transmit = _ptr(grad_depth), _ptr(grad_logt)
    a.tape = 0 if grad_depth is None else tape.data_ptr()
    a.grad_density = gd.data_ptr()
    a.use_skip = 1
    a.stream = g.ctx.stream().value
    check(g.ctx.lib.nerf_grid_depth_backward(h, C.byref(opt._to_c()), C.byref(a)))


class _VolumeRenderDepth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, density, module, o, d):
        g = module.grid
        opt = replace(g.opt)
        h = g._handle()
        n = o.shape[0]
        depth = torch.empty((n,), device=o.device, dtype=torch.float32)
        logt = torch.empty((n,), device=o.device, dtype=torch.float32)
        tape = torch.empty((n,), device=o.device, dtype=torch.float64)
        a = GridDepthTapedArgs()
        a.origins, a.dirs, a.n_rays = o.data_ptr(), d.data_ptr(), n
        a.depth, a.log_transmit, a.tape = depth.data_ptr(), logt.data_ptr(), tape.data_ptr()
        a.use_skip = 1
        a.stream = g.ctx.stream().value
        check(g.ctx.lib.nerf_grid_depth_rays_taped(h, C.byref(opt._to_c()), C.byref(a)))
        ctx.save_for_backward(density, o, d, tape)
        ctx.module, ctx.opt = module, opt
        ctx.set_materialize_grads(False)
        return depth, logt

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_depth, grad_logt):
        density, o, d, tape = ctx.saved_tensors
        g = ctx.module.grid
        h = _same_tables(ctx.module, density)
        gd = torch.zeros_like(density, memory_format=torch.contiguous_format)
        if grad_depth is not None or grad_logt is not None:
            _depth_backward(g, h, ctx.opt, o, d, grad_depth, grad_logt, tape, gd)
        return gd, None, None, None


class _Sample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, density, sh, module, p, grid_coords, want_colors):
        out_density, out_sh = module.grid.sample(p, grid_coords=grid_coords, want_colors=want_colors)
        ctx.save_for_backward(density, sh, p)
        ctx.module, ctx.grid_coords, ctx.want_colors = module, grid_coords, want_colors
        if not want_colors:
            ctx.mark_non_differentiable(out_sh)
        return out_density, out_sh

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_density_out, grad_sh_out):
        density, sh, p = ctx.saved_tensors
        g = ctx.module.grid
        h = _same_tables(ctx.module, density, sh)
        gd = _zeros_like_or_none(density, ctx.needs_input_grad[0])
        gs = _zeros_like_or_none(sh, ctx.needs_input_grad[1] and ctx.want_colors)
        go_d = grad_density_out.to(dtype=torch.float32).contiguous()
        go_s = grad_sh_out.to(dtype=torch.float32).contiguous() if ctx.want_colors else None
        a = GridSampleBackwardArgs()
        a.points, a.n = p.data_ptr(), p.shape[0]
        a.grid_coords, a.want_colors = int(ctx.grid_coords), int(ctx.want_colors)
        a.grad_out_density, a.grad_out_sh = go_d.data_ptr(), _ptr(go_s)
        a.grad_density, a.grad_sh = _ptr(gd), _ptr(gs)
        a.stream = g.ctx.stream().value
        check(g.ctx.lib.nerf_grid_sample_backward(h, C.byref(a)))
        return gd, gs, None, None, None, None      # (without want_colors sh_data takes no part: no gradient)


def _cells_arg(cells, device):
    """``cells`` as a contiguous 1-D int32 / int64 tensor on ``device`` (None stays None: the dense form)"""
    if cells is None:
        return None
    if not torch.is_tensor(cells):
        raise TypeError("cells must be a tensor")
    if cells.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"cells must be int32 or int64, got {cells.dtype}")
    if not cells.is_cuda:
        raise RuntimeError("cells is on the CPU: GridModule has no CPU fallback")
    if cells.dim() != 1:
        raise ValueError(f"cells must be [M] flat node indices, got {tuple(cells.shape)}")
    return cells.detach().to(device=device).contiguous()


def _tv_args(g, target, start_dim, end_dim, ignore_edge, cells):
    a = GridTvValueArgs()
    a.target, a.start_dim, a.end_dim, a.ignore_edge = target, start_dim, end_dim, int(ignore_edge)
    if cells is not None:
        # (an empty tensor has no address: any non-NULL one says "a list", and none of its entries is read)
        a.cells, a.cells_int64, a.n_cells = cells.data_ptr() or g.links.data_ptr(), int(cells.dtype == torch.int64), cells.shape[0]
    a.stream = g.ctx.stream().value
    return a


def _tv_value(g, h, target, start_dim, end_dim, ignore_edge, cells):
    """nerf_grid_tv_value: the 0-dim fp32 value; the partials are a workspace of this call"""
    dev = g.ctx.device
    n = cells.shape[0] if cells is not None else (g.links.shape[0] - 1) * (g.links.shape[1] - 1) * (g.links.shape[2] - 1)
    work = torch.empty((int(g.ctx.lib.nerf_grid_tv_value_workspace(n * (end_dim - start_dim))),), device=dev, dtype=torch.float64)
    value = torch.empty((), device=dev, dtype=torch.float32)
    a = _tv_args(g, target, start_dim, end_dim, ignore_edge, cells)
    a.partials, a.value = work.data_ptr(), value.data_ptr()
    check(g.ctx.lib.nerf_grid_tv_value(h, C.byref(a)))
    return value, n


class _TotalVariation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, module, target, start_dim, end_dim, ignore_edge, cells):
        g = module.grid
        value, n = _tv_value(g, g._handle(), target, start_dim, end_dim, ignore_edge, cells)
        ctx.save_for_backward(table)      # the parameter: torch refuses a backward after an in-place step
        ctx.module, ctx.cells, ctx.call = module, cells, (target, start_dim, end_dim, ignore_edge)
        ctx.items = n * (end_dim - start_dim)
        return value

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_value):
        (table,) = ctx.saved_tensors
        g = ctx.module.grid
        if ctx.call[0] == NERF_GRID_TV_DENSITY:
            h = _same_tables(ctx.module, table)
        else:
            h = _same_tables(ctx.module, g.density_data, table)
        if ctx.items == 0:      # no cell or no column: the value is the constant 0
            return None, None, None, None, None, None, None
        grad = torch.zeros_like(table, memory_format=torch.contiguous_format)
        grad_value = grad_value.to(dtype=torch.float32).contiguous()      # stays on the device: the kernel reads it
        a = _tv_args(g, *ctx.call, ctx.cells)
        a.grad_value, a.grad = grad_value.data_ptr(), grad.data_ptr()
        check(g.ctx.lib.nerf_grid_tv_value_backward(h, C.byref(a)))
        return grad, None, None, None, None, None, None


def _sparsity_args(g, o, d):
    a = GridSparsityArgs()
    a.origins, a.dirs, a.n_rays = o.data_ptr(), d.data_ptr(), o.shape[0]
    a.use_skip = 1
    a.stream = g.ctx.stream().value
    return a


def _sparsity_rays(g, h, opt, o, d):
    s = torch.empty((o.shape[0],), device=o.device, dtype=torch.float32)
    a = _sparsity_args(g, o, d)
    a.sparsity = s.data_ptr()
    check(g.ctx.lib.nerf_grid_sparsity_rays(h, C.byref(opt._to_c()), C.byref(a)))
    return s


class _SparsityLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, density, module, o, d):
        g = module.grid
        opt = replace(g.opt)
        s = _sparsity_rays(g, g._handle(), opt, o, d)
        ctx.save_for_backward(density, o, d)      # nothing is kept per ray besides the rays themselves
        ctx.module, ctx.opt = module, opt
        return s

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_s):
        density, o, d = ctx.saved_tensors
        g = ctx.module.grid
        h = _same_tables(ctx.module, density)
        gd = torch.zeros_like(density, memory_format=torch.contiguous_format)
        if o.shape[0]:
            grad_s = grad_s.to(dtype=torch.float32).contiguous()      # (s.sum().backward() hands in a stride-0 expansion)
            a = _sparsity_args(g, o, d)
            a.grad_sparsity, a.grad_density = grad_s.data_ptr(), gd.data_ptr()
            check(g.ctx.lib.nerf_grid_sparsity_backward(h, C.byref(ctx.opt._to_c()), C.byref(a)))
        return gd, None, None, None


class GridModule(torch.nn.Module):
    """``density_data`` and ``sh_data`` are ``nn.Parameter`` views of the grid's own tensors: the same storage and the same
    version counter, so an optimiser that steps them in place is seen by ``grid.volume_render_image`` at once - the grid's
    handle stays, and so does its skip data, which depends on ``links`` only. The grid's attributes stay plain tensors.

    If the grid's tables are replaced (``GridTrainer.resample`` / ``remove_floaters``, or assignment) the next call raises a
    ``RuntimeError`` that names :meth:`rebind`, which makes new parameters; optimiser state built on the old ones is the
    caller's business. ``self.grid.opt`` are the render options, read at every forward.

    Under ``torch.no_grad()``, or with both parameters frozen (for a depth: with ``density_data`` frozen), the methods call
    the plain kernels and keep no tape."""

    def __init__(self, grid: SparseGrid):
        super().__init__()
        _refuse_half(grid, "GridModule")
        if not isinstance(grid, SparseGrid):
            raise TypeError("GridModule needs a SparseGrid")
        self.grid = grid
        self.rebind()

    def rebind(self):
        """Make ``density_data`` / ``sh_data`` anew from the grid's current tensors (``requires_grad`` as before, or True)."""
        g = self.grid
        g._handle()      # validates the tensors
        old = [getattr(self, name, None) for name in ("density_data", "sh_data")]
        self._bound = (g.density_data, g.sh_data)
        self.density_data = torch.nn.Parameter(g.density_data, requires_grad=old[0] is None or old[0].requires_grad)
        self.sh_data = torch.nn.Parameter(g.sh_data, requires_grad=old[1] is None or old[1].requires_grad)
        return self

    def _check_bound(self):
        g = self.grid
        pairs = ((g.density_data, self._bound[0], self.density_data), (g.sh_data, self._bound[1], self.sh_data))
        for now, bound, param in pairs:
            if now is not bound or param.data_ptr() != now.data_ptr() or param.shape != now.shape:
                raise RuntimeError("the grid's density_data / sh_data are no longer the tensors this GridModule's parameters "
                                   "were made from: call rebind() (and make the optimiser anew)")

    def _differentiate(self):
        return torch.is_grad_enabled() and (self.density_data.requires_grad or self.sh_data.requires_grad)

    def volume_render(self, rays: Rays, use_kernel: bool = True, return_log_transmit: bool = False):
        """``[N, 3]``, bit-identical to ``grid.volume_render(rays)``, differentiable with respect to the parameters. With
        ``return_log_transmit``: ``(rgb, log_transmit [N])``, both differentiable (``log_transmit`` with respect to
        ``density_data``; exactly -1e3, with no gradient, where a ray stopped at ``stop_thresh``)."""
        if not use_kernel:
            raise NotImplementedError("use_kernel=False (the PyTorch renderer) does not exist here: HIP kernels only")
        self._check_bound()
        dev = self.grid.ctx.device
        o = _points_arg(rays.origins, "rays.origins", dev)
        d = _points_arg(rays.dirs, "rays.dirs", dev, o.shape[0])
        if not self._differentiate():
            return self.grid.volume_render(Rays(o, d), return_log_transmit=return_log_transmit)
        rgb, logt = _VolumeRender.apply(self.density_data, self.sh_data, self, o, d, bool(return_log_transmit))
        return (rgb, logt) if return_log_transmit else rgb

    def volume_render_depth(self, rays: Rays, sigma_thresh=None, return_log_transmit: bool = False):
        """``[N]`` as ``grid.volume_render_depth``, bit for bit. The expected termination (``sigma_thresh=None``) and, with
        ``return_log_transmit``, ``log_transmit [N]`` are differentiable with respect to ``density_data``: one backward
        launch takes both cotangents; ``sh_data`` takes no part. The threshold depth (``sigma_thresh=x``) is piecewise
        constant: the plain kernel's result, which does not require grad."""
        mode, _ = SparseGrid._depth_mode(sigma_thresh, return_log_transmit)
        self._check_bound()
        dev = self.grid.ctx.device
        o = _points_arg(rays.origins, "rays.origins", dev)
        d = _points_arg(rays.dirs, "rays.dirs", dev, o.shape[0])
        if mode != NERF_GRID_DEPTH_EXPECTED or not (torch.is_grad_enabled() and self.density_data.requires_grad):
            return self.grid.volume_render_depth(Rays(o, d), sigma_thresh=sigma_thresh, return_log_transmit=return_log_transmit)
        depth, logt = _VolumeRenderDepth.apply(self.density_data, self, o, d)
        return (depth, logt) if return_log_transmit else depth

    def volume_render_depth_image(self, camera: Camera, sigma_thresh=None, return_log_transmit: bool = False):
        """``[H, W]`` (with ``return_log_transmit`` a pair of them): :meth:`volume_render_depth` of ``camera.gen_rays()``,
        bit-identical to ``grid.volume_render_depth_image``."""
        SparseGrid._depth_mode(sigma_thresh, return_log_transmit)      # a bad threshold is refused before anything else
        out = self.volume_render_depth(camera.gen_rays(self.grid.ctx.device), sigma_thresh, return_log_transmit)
        if return_log_transmit:
            return tuple(t.view(camera.height, camera.width) for t in out)
        return out.view(camera.height, camera.width)

    def volume_render_image(self, camera: Camera, use_kernel: bool = True):
        """``[H, W, 3]``: :meth:`volume_render` of ``camera.gen_rays()``, bit-identical to ``grid.volume_render_image``."""
        if not use_kernel:
            raise NotImplementedError("use_kernel=False (the PyTorch renderer) does not exist here: HIP kernels only")
        return self.volume_render(camera.gen_rays(self.grid.ctx.device)).view(camera.height, camera.width, 3)

    def sample(self, points: torch.Tensor, use_kernel: bool = True, grid_coords: bool = False, want_colors: bool = True):
        """``(density [N, 1], sh [N, 3 * basis_dim])`` as ``grid.sample``, differentiable with respect to the parameters."""
        if not use_kernel:
            raise NotImplementedError("use_kernel=False (the PyTorch sampler) does not exist here: HIP kernels only")
        self._check_bound()
        p = _points_arg(points, "points", self.grid.ctx.device)
        if not self._differentiate():
            return self.grid.sample(p, grid_coords=grid_coords, want_colors=want_colors)
        return _Sample.apply(self.density_data, self.sh_data, self, p, bool(grid_coords), bool(want_colors))

    def _tv(self, target, start_dim, end_dim, ignore_edge, cells):
        g = self.grid
        param = self.density_data if target == NERF_GRID_TV_DENSITY else self.sh_data
        _refuse_half(g, "GridModule.tv / tv_color")
        self._check_bound()
        cells = _cells_arg(cells, g.ctx.device)
        if not (torch.is_grad_enabled() and param.requires_grad):
            return _tv_value(g, g._handle(), target, start_dim, end_dim, ignore_edge, cells)[0]
        return _TotalVariation.apply(param, self, target, start_dim, end_dim, ignore_edge, cells)

    def tv(self, cells: torch.Tensor = None, logalpha: bool = False, logalpha_delta: float = 2.0, ndc_coeffs=(-1.0, -1.0)):
        """svox2's ``SparseGrid.tv()``: the total variation of the densities, a 0-dim fp32 tensor, differentiable with respect
        to ``density_data`` only - the mean over cells of ``sqrt(1e-5 + dx^2 + dy^2 + dz^2)`` of the forward differences
        scaled by ``reso / 256``, an empty node counting as 0. ``cells=None``: every cell with three forward neighbours.
        ``cells``: an int32 / int64 device tensor of flat C-order node indices (svox2's ``_get_rand_cells``), duplicates
        counting as often as they appear, entries outside the lattice contributing 0; the divisor is ``len(cells)``. Two
        calls return the same bits. The gradient is the exact gradient of this value times the cotangent, which is NOT what
        svox2's ``_TotalVariationFunction.backward`` computes (include/nerf_mi355x.h, ``nerf_grid_tv_value_backward``).
        ``ndc_coeffs`` is accepted and has no effect, as in svox2, whose NDC branch of ``calculate_ray_scale`` is commented
        out; ``logalpha=True`` raises."""
        if logalpha:
            raise NotImplementedError("logalpha=True is not built: svox2 itself asserts 'No longer supported'")
        return self._tv(NERF_GRID_TV_DENSITY, 0, 1, False, cells)

    def tv_color(self, start_dim: int = 0, end_dim: int = None, cells: torch.Tensor = None, logalpha: bool = False,
                 logalpha_delta: float = 2.0, ndc_coeffs=(-1.0, -1.0)):
        """svox2's ``SparseGrid.tv_color()``: :meth:`tv` of columns ``[start_dim, end_dim)`` of ``sh_data`` (negative values
        wrap as in svox2), summed over the columns, differentiable with respect to ``sh_data`` only, with svox2's
        ``ignore_edge``: an empty or out-of-range neighbour takes the cell's own value, and the cell whose link is row 0 is
        left out. ``start_dim == end_dim`` is the constant 0. ``ndc_coeffs`` is accepted and has no effect, as in svox2."""
        if logalpha:
            raise NotImplementedError("logalpha=True is not built: svox2 itself asserts 'No longer supported'")
        cols = self.sh_data.shape[1]
        end_dim = cols if end_dim is None else int(end_dim)
        start_dim = int(start_dim)
        end_dim = end_dim + cols if end_dim < 0 else end_dim
        start_dim = start_dim + cols if start_dim < 0 else start_dim
        if not 0 <= start_dim <= end_dim <= cols:
            raise ValueError(f"columns [{start_dim}, {end_dim}) outside [0, {cols})")
        return self._tv(NERF_GRID_TV_SH, start_dim, end_dim, True, cells)

    def sparsity_loss(self, rays: Rays):
        """``[N]``: per ray the sum of ``log(1 + 2 sigma^2)`` over the samples of the renderer's own march that it shades
        (``sigma > sigma_thresh``, up to and including the sample at which ``stop_thresh`` ends the ray); exactly 0 for a ray
        that is not marched. Differentiable with respect to ``density_data`` only. It is the function whose gradient
        ``GridTrainer.volume_render_fused(..., sparsity_loss=l)`` adds: write ``l * m.sparsity_loss(rays).sum()``."""
        g = self.grid
        _refuse_half(g, "GridModule.sparsity_loss")
        self._check_bound()
        o = _points_arg(rays.origins, "rays.origins", g.ctx.device)
        d = _points_arg(rays.dirs, "rays.dirs", g.ctx.device, o.shape[0])
        if not (torch.is_grad_enabled() and self.density_data.requires_grad):
            return _sparsity_rays(g, g._handle(), g.opt, o, d)
        return _SparsityLoss.apply(self.density_data, self, o, d)

    def forward(self, rays: Rays):
        return self.volume_render(rays)
