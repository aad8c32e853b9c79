"""Training a sparse voxel grid (Plenoxels): fused render + MSE backward, total-variation gradients, RMSProp / SGD.

``GridTrainer(grid)`` optimises a :class:`~nerf_projects_amd.grid.SparseGrid` in place through the HIP kernels of
csrc/grid_train_kernels.hip; the semantics of every call are stated in include/nerf_mi355x.h, "Sparse voxel grid:
training". It is the counterpart of svox2's training loop under names of its own::

    svox2                                              here
    grid.volume_render_fused(rays, rgb_gt)             trainer.forward_backward(rays, rgb_gt)
    grid.volume_render_fused(rays, rgb_gt,             trainer.volume_render_fused(rays, rgb_gt,
        beta_loss=..., sparsity_loss=...)                  beta_loss=..., sparsity_loss=...)
    grid.inplace_tv_grad(grid.density_data.grad, ...)  trainer.add_tv_grad("density", ...)
    grid.inplace_tv_color_grad(grid.sh_data.grad, ...) trainer.add_tv_grad("sh", ..., ignore_edge=True)
    grid.optim_density_step / grid.optim_sh_step       trainer.step(lr_sigma, lr_sh, ...)
    grid.resample(reso, ...)                           trainer.resample(reso, ...)      (grid_resample.py)
    (nothing)                                          trainer.remove_floaters(...)     (grid_components.py)

The svox2-named methods on ``SparseGrid`` itself still raise ``NotImplementedError``. There is no PyTorch fallback: the
gradients are not autograd tensors, they live in ``trainer.grad_density`` / ``trainer.grad_sh``.
"""
import ctypes as C
import math

import torch

from ._lib import (NERF_GRID_OPTIM_RMSPROP, NERF_GRID_OPTIM_SGD, NERF_GRID_TV_DENSITY, NERF_GRID_TV_SH, GridFusedArgs,
                   GridOptimArgs, GridTvArgs, check)
from .grid import Rays, SparseGrid, _refuse_half

__all__ = ["GridTrainer"]


class GridTrainer:
    """Owns what training adds to a grid: ``grad_density`` ``[capacity, 1]``, ``grad_sh`` ``[capacity, 3 * basis_dim]``,
    ``mask`` ``[capacity]`` (uint8: the rows a step touches, svox2's ``sparse_grad_indexer``), and the RMSProp state
    ``density_rms`` / ``sh_rms``. The grid's ``density_data`` / ``sh_data`` are updated in place, so the grid's handle and
    its skip data (which depend on ``links`` only) stay valid across steps. Replacing the grid's tensors with ones of another
    capacity after the trainer was made is an error at the next call; :meth:`resample` is how a training loop changes the
    resolution and the kept nodes.

    ``generator``: a CPU ``torch.Generator`` from which :meth:`add_tv_grad` draws the start of its cell range."""

    def __init__(self, grid: SparseGrid, generator: torch.Generator = None):
        _refuse_half(grid, "GridTrainer")
        if not isinstance(grid, SparseGrid):
            raise TypeError("GridTrainer needs a SparseGrid")
        self.grid = grid
        self.ctx = grid.ctx
        grid._handle()      # validates the tensors
        self._allocate()
        self.generator = generator if generator is not None else torch.Generator(device="cpu")

    def _check_capacity(self):
        g = self.grid
        if tuple(g.density_data.shape) != tuple(self.grad_density.shape) or tuple(g.sh_data.shape) != tuple(self.grad_sh.shape):
            raise ValueError(f"the grid's tables changed shape since this trainer was made: density_data "
                             f"{tuple(g.density_data.shape)}, sh_data {tuple(g.sh_data.shape)}; gradients "
                             f"{tuple(self.grad_density.shape)}, {tuple(self.grad_sh.shape)}")

    def _allocate(self):
        dev = self.ctx.device
        cap, cols = self.grid.density_data.shape[0], self.grid.sh_data.shape[1]
        self.grad_density = torch.zeros((cap, 1), dtype=torch.float32, device=dev)
        self.grad_sh = torch.zeros((cap, cols), dtype=torch.float32, device=dev)
        self.mask = torch.zeros((cap,), dtype=torch.uint8, device=dev)
        self.density_rms = torch.zeros((cap, 1), dtype=torch.float32, device=dev)
        self.sh_rms = torch.zeros((cap, cols), dtype=torch.float32, device=dev)

    def _replace_tables(self, new: SparseGrid, accelerate: bool):
        """The tables of ``new`` (made from this trainer's grid, so every argument has been accepted) replace the grid's in
        place; the training state is allocated anew and zeroed; the handle, and with ``accelerate`` the skip data, are rebuilt."""
        g = self.grid
        g.links, g.density_data, g.sh_data = new.links, new.density_data, new.sh_data
        self._allocate()
        if accelerate:
            g.accelerate()
        else:
            g._handle()

    def resample(self, reso, sigma_thresh: float = 5.0, weight_thresh: float = 0.01, dilate: int = 2, cameras=None,
                 accelerate: bool = True, weight_render_stop_thresh: float = 0.2, max_elements: int = 0):
        """svox2's ``grid.resample`` inside a training loop: :func:`~nerf_projects_amd.grid_resample.resample_grid` of the
        trainer's grid, whose ``links``, ``density_data`` and ``sh_data`` are then replaced in place (the old handle and its
        skip data are dropped; with ``accelerate`` the skip data is built again). The gradients, the mask and the RMSProp
        state are allocated anew at the new capacity and zeroed, as svox2 resets them. An argument error leaves the grid and
        the trainer as they were."""
        from .grid_resample import resample_grid
        self._check_capacity()
        self._replace_tables(resample_grid(self.grid, reso, sigma_thresh, weight_thresh, dilate, cameras, False,
                                           weight_render_stop_thresh, max_elements), accelerate)

    def remove_floaters(self, accelerate: bool = True, **fdr_kwargs):
        """:func:`~nerf_projects_amd.grid_components.remove_floaters` inside a training loop, with the contract of
        :meth:`resample`: the grid's ``links``, ``density_data`` and ``sh_data`` are replaced in place by those without the
        floater components (kept rows bit for bit), the old handle and its skip data are dropped (with ``accelerate`` the
        skip data is built again), and the gradients, the mask and the RMSProp state are allocated anew and zeroed. Returns
        the ``compute_FDR`` result of the grid as it was. An argument error leaves the grid and the trainer as they were."""
        from .grid_components import remove_floaters
        self._check_capacity()
        new, result = remove_floaters(self.grid, False, **fdr_kwargs)
        self._replace_tables(new, accelerate)
        return result

    def zero_grad(self):
        """Zero both gradients and the mask (the kernels accumulate)."""
        self.grad_density.zero_()
        self.grad_sh.zero_()
        self.mask.zero_()

    def forward_backward(self, rays: Rays, rgb_gt: torch.Tensor, beta_loss: float = 0.0, sparsity_loss: float = 0.0,
                         randomize: bool = False, return_log_transmit: bool = False):
        """Render ``rays`` (``rgb_out [N, 3]``, bit-identical to ``grid.volume_render(rays)``) and add the gradients of
        ``mean((rgb_out - rgb_gt) ** 2)`` to ``grad_density`` / ``grad_sh``, marking the touched rows in ``mask``.
        ``beta_loss`` and ``sparsity_loss`` are refused here: :meth:`volume_render_fused` has them."""
        if beta_loss:
            raise NotImplementedError("beta_loss is not built in forward_backward: use volume_render_fused")
        if sparsity_loss:
            raise NotImplementedError("sparsity_loss is not built in forward_backward: use volume_render_fused")
        return self._fused(rays, rgb_gt, 0.0, 0.0, randomize, return_log_transmit, "nerf_grid_fused_backward")

    def volume_render_fused(self, rays: Rays, rgb_gt: torch.Tensor, randomize: bool = False, beta_loss: float = 0.0,
                            sparsity_loss: float = 0.0, return_log_transmit: bool = False):
        """svox2's ``grid.volume_render_fused``: :meth:`forward_backward` plus the two regularisers of its published
        configurations, folded into the density gradient of the same march. ``beta_loss`` is ``opt.py``'s ``lambda_beta``:
        the kernel receives it divided by the number of rays, as svox2's does, and adds the gradient of
        ``(beta_loss / N) * sum_ray [log_T + log(1 - exp(log_T) + 1e-3)]``. ``sparsity_loss`` is ``lambda_sparsity``, passed as
        given: the gradient of ``sparsity_loss * sum over shaded samples of log(1 + 2 sigma ** 2)``. Both are finite and
        ``>= 0``; ``rgb_out``, ``grad_sh`` and ``mask`` do not depend on them. ``randomize=True`` is refused."""
        for name, v in (("beta_loss", beta_loss), ("sparsity_loss", sparsity_loss)):
            if not (math.isfinite(v) and v >= 0.0):
                raise ValueError(f"{name} = {v} must be finite and >= 0")
        if randomize:
            raise NotImplementedError("randomize is not built")
        return self._fused(rays, rgb_gt, float(beta_loss), float(sparsity_loss), False, return_log_transmit,
                           "nerf_grid_fused_backward_losses")

    def _fused(self, rays, rgb_gt, lambda_beta, sparsity_loss, randomize, return_log_transmit, entry):
        g = self.grid
        self._check_capacity()
        opt = g.opt._to_c(randomize)
        o = g._rays_arg(rays.origins, "rays.origins")
        d = g._rays_arg(rays.dirs, "rays.dirs", o.shape[0])
        n = o.shape[0]
        if not torch.is_tensor(rgb_gt):
            raise TypeError("rgb_gt must be a tensor")
        if not rgb_gt.is_cuda:
            raise RuntimeError("rgb_gt is on the CPU: SparseGrid has no CPU fallback")
        if rgb_gt.dim() != 2 or tuple(rgb_gt.shape) != (n, 3):
            raise ValueError(f"rgb_gt must be [{n}, 3] like the rays, got {tuple(rgb_gt.shape)}")
        gt = rgb_gt.detach().to(device=self.ctx.device, dtype=torch.float32).contiguous()
        h = g._handle()
        rgb = torch.empty((n, 3), device=self.ctx.device, dtype=torch.float32)
        logt = torch.empty((n,), device=self.ctx.device, dtype=torch.float32) if return_log_transmit else None
        a = GridFusedArgs()
        a.origins, a.dirs, a.rgb_gt, a.n_rays = o.data_ptr(), d.data_ptr(), gt.data_ptr(), n
        a.rgb_out = rgb.data_ptr()
        a.log_transmit = 0 if logt is None else logt.data_ptr()
        a.grad_density, a.grad_sh, a.mask = self.grad_density.data_ptr(), self.grad_sh.data_ptr(), self.mask.data_ptr()
        a.beta_loss, a.sparsity_loss = lambda_beta / max(n, 1), sparsity_loss      # (svox2 divides lambda_beta by the rays too)
        a.use_skip = 1
        a.stream = self.ctx.stream().value
        check(getattr(self.ctx.lib, entry)(h, C.byref(opt), C.byref(a)))
        return (rgb, logt) if return_log_transmit else rgb

    def add_tv_grad(self, target: str = "density", scaling: float = 1.0, sparse_frac: float = 0.01, start: int = None,
                    start_dim: int = 0, end_dim: int = None, ignore_edge: bool = False):
        """Add the gradient of svox2's total-variation loss over ``max(1, int(sparse_frac * X Y Z))`` nodes starting at node
        ``start`` (C order, wrapping past the last; drawn from ``self.generator`` when ``None``) to the gradient of the
        ``"density"`` or the ``"sh"`` table, columns ``[start_dim, end_dim)``. The kernel receives
        ``scaling / count`` as svox2's does. ``ignore_edge=True`` is the rule svox2's ``inplace_tv_color_grad`` always runs
        with: an empty or out-of-range neighbour takes the cell's own value (no pull towards 0 at the shell of a sparse
        grid), and the cell whose link is row 0 is left out (include/nerf_mi355x.h, ``nerf_grid_tv_grad_edge``). Returns
        ``(start, count)``."""
        g = self.grid
        self._check_capacity()
        if target not in ("density", "sh"):
            raise ValueError(f"target {target!r}: 'density' or 'sh'")
        n = g.links.numel()
        cols = 1 if target == "density" else g.sh_data.shape[1]
        end_dim = cols if end_dim is None else int(end_dim)
        start_dim = int(start_dim)
        if not 0 <= start_dim <= end_dim <= cols:
            raise ValueError(f"columns [{start_dim}, {end_dim}) outside [0, {cols})")
        if not 0.0 < sparse_frac <= 1.0:
            raise ValueError(f"sparse_frac = {sparse_frac} must be in (0, 1]")
        count = max(1, int(sparse_frac * n))
        if start is None:
            start = int(torch.randint(0, n, (1,), generator=self.generator).item())
        if not 0 <= start < n:
            raise ValueError(f"start = {start} outside [0, {n})")
        a = GridTvArgs()
        a.target = NERF_GRID_TV_DENSITY if target == "density" else NERF_GRID_TV_SH
        a.start_dim, a.end_dim, a.start, a.count = start_dim, end_dim, start, count
        a.scale = float(scaling) / count
        a.ignore_edge = 1 if ignore_edge else 0
        a.grad = (self.grad_density if target == "density" else self.grad_sh).data_ptr()
        a.mask = self.mask.data_ptr()
        a.stream = self.ctx.stream().value
        entry = self.ctx.lib.nerf_grid_tv_grad_edge if ignore_edge else self.ctx.lib.nerf_grid_tv_grad
        check(entry(g._handle(), C.byref(a)))
        return start, count

    def _step_one(self, data, rms, grad, kind, beta, lr, eps, minval):
        a = GridOptimArgs()
        a.data, a.rms, a.grad, a.mask = data.data_ptr(), rms.data_ptr(), grad.data_ptr(), self.mask.data_ptr()
        a.rows, a.cols, a.kind = data.shape[0], data.shape[1], kind
        a.beta, a.lr, a.eps, a.minval = beta, lr, eps, minval
        a.stream = self.ctx.stream().value
        check(self.ctx.lib.nerf_grid_optim_step(self.ctx.handle, C.byref(a)))

    def step(self, lr_sigma: float, lr_sh: float, beta: float = 0.95, epsilon: float = 1e-8, optim: str = "rmsprop",
             minval: float = -1e9):
        """One masked optimiser step on both tables (svox2's ``optim_density_step`` and ``optim_sh_step``): rows whose mask
        byte is unset, and their ``rms``, are untouched. The gradients and the mask are left as they are."""
        g = self.grid
        self._check_capacity()
        if optim not in ("rmsprop", "sgd"):
            raise ValueError(f"optim {optim!r}: 'rmsprop' or 'sgd'")
        g._handle()      # the tables are validated (GPU, fp32, contiguous) before anything writes through their pointers
        kind = NERF_GRID_OPTIM_RMSPROP if optim == "rmsprop" else NERF_GRID_OPTIM_SGD
        self._step_one(g.density_data, self.density_rms, self.grad_density, kind, beta, lr_sigma, epsilon, minval)
        self._step_one(g.sh_data, self.sh_rms, self.grad_sh, kind, beta, lr_sh, epsilon, minval)

    def train_step(self, rays: Rays, rgb_gt: torch.Tensor, lr_sigma: float = 30.0, lr_sh: float = 1e-2, beta: float = 0.95,
                   epsilon: float = 1e-8, optim: str = "rmsprop", lambda_tv: float = 0.0, lambda_tv_sh: float = 0.0,
                   tv_sparsity: float = 0.01, lambda_beta: float = 0.0, lambda_sparsity: float = 0.0,
                   tv_sh_ignore_edge: bool = False):
        """``zero_grad``, ``forward_backward`` (``volume_render_fused`` where ``lambda_beta`` or ``lambda_sparsity`` is not
        zero), the TV gradients whose weight is not zero, ``step``. ``tv_sh_ignore_edge=True`` is what svox2's colour TV does.
        Returns ``{"mse", "psnr"}`` of the batch before the step (reading them waits for the device)."""
        self.zero_grad()
        if lambda_beta or lambda_sparsity:
            rgb = self.volume_render_fused(rays, rgb_gt, beta_loss=lambda_beta, sparsity_loss=lambda_sparsity)
        else:
            rgb = self.forward_backward(rays, rgb_gt)
        if lambda_tv:
            self.add_tv_grad("density", lambda_tv, tv_sparsity)
        if lambda_tv_sh:
            self.add_tv_grad("sh", lambda_tv_sh, tv_sparsity, ignore_edge=tv_sh_ignore_edge)
        self.step(lr_sigma, lr_sh, beta, epsilon, optim)
        gt = rgb_gt.detach().to(device=rgb.device, dtype=torch.float32)
        mse = float(((rgb - gt) ** 2).mean()) if rgb.numel() else float("nan")
        return {"mse": mse, "psnr": -10.0 * math.log10(mse) if mse > 0 else float("inf")}
