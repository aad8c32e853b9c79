"""Training a sparse voxel grid together with its background layers: ``BackgroundTrainer(grid)`` optimises a
:class:`~nerf_projects_amd.grid_background.BackgroundGrid` in place - the foreground tables as ``GridTrainer`` does, and
``background_data`` through the HIP kernels of csrc/grid_background_train_kernels.hip. The semantics of every call are stated
in include/nerf_mi355x.h, "Sparse voxel grid: background layers, training". The four background steps of svox2's
optimisation loop under names of their own::

    svox2                                                        here
    grid.volume_render_fused(rays, rgb_gt)                       trainer.forward_backward(rays, rgb_gt)
    grid.volume_render_fused(rays, rgb_gt, beta_loss=...,        trainer.volume_render_fused(rays, rgb_gt, beta_loss=...,
        sparsity_loss=...)                                           sparsity_loss=...)      (sparsity: foreground samples only)
    grid.inplace_tv_background_grad(grid.background_data.grad)   trainer.add_tv_grad("background", ...)
    grid.optim_background_step(lr_sigma_bg, lr_color_bg, ...)    trainer.step(..., lr_sigma_bg, lr_color_bg, ...)
    grid.sparsify_background(...)                                trainer.sparsify_background(...)

The foreground's gradients are complete here: the density gradient of a sample contains what lies behind it, the background
included (the fp64 tape of the foreground render and of the background pass are added before the foreground's backward
starts from it). There is no PyTorch fallback: the gradients are not autograd tensors, they live in ``trainer.grad_density``,
``trainer.grad_sh`` and ``trainer.grad_background``.
"""
import ctypes as C
import math

import numpy as np
import torch

from ._lib import (NERF_GRID_OPTIM_RMSPROP, NERF_GRID_OPTIM_SGD, GridBackgroundBackwardArgs, GridBackgroundOptimArgs,
                   GridBackgroundTapedArgs, GridBackgroundTvArgs, GridRenderBackwardArgs, GridRenderBackwardLossesArgs,
                   GridRenderTapedArgs, check)
from .grid import Rays
from .grid_background import BackgroundGrid
from .grid_train import GridTrainer

__all__ = ["BackgroundTrainer"]


class BackgroundTrainer:
    """Owns what training adds to a ``BackgroundGrid``: the state of a ``GridTrainer`` on ``grid.foreground()``'s tensors
    (``grad_density``, ``grad_sh``, ``mask``, ``density_rms``, ``sh_rms``) and, for the layers, ``grad_background``
    ``[capacity, L, 4]``, ``mask_background`` ``[capacity, L]`` (uint8: the (row, layer) entries a step touches) and
    ``background_rms``. All tables are updated in place, so the grid's handle, its skip data and the attached background stay
    valid across steps and renders see the trained values. A table of another shape than the state's (after an assignment to
    the grid) is an error at the next call; :meth:`resample`, :meth:`remove_floaters` and :meth:`sparsify_background` are how a
    training loop changes the shapes.

    ``generator``: a CPU ``torch.Generator`` from which :meth:`add_tv_grad` draws the start of its cell range."""

    def __init__(self, grid: BackgroundGrid, generator: torch.Generator = None):
        if not isinstance(grid, BackgroundGrid):
            raise TypeError("BackgroundTrainer needs a BackgroundGrid (a SparseGrid without layers trains with GridTrainer)")
        self.grid = grid
        self.ctx = grid.ctx
        grid._handle()      # validates the tensors
        self.generator = generator if generator is not None else torch.Generator(device="cpu")
        self._fg = GridTrainer(grid.foreground(), self.generator)
        self._allocate_background()

    # ---- state ----------------------------------------------------------------------------------------------
    grad_density = property(lambda self: self._fg.grad_density)
    grad_sh = property(lambda self: self._fg.grad_sh)
    mask = property(lambda self: self._fg.mask)
    density_rms = property(lambda self: self._fg.density_rms)
    sh_rms = property(lambda self: self._fg.sh_rms)

    def _allocate_background(self):
        dev = self.ctx.device
        cap, nl = self.grid.background_data.shape[0], self.grid.background_data.shape[1]
        self.grad_background = torch.zeros((cap, nl, 4), dtype=torch.float32, device=dev)
        self.mask_background = torch.zeros((cap, nl), dtype=torch.uint8, device=dev)
        self.background_rms = torch.zeros((cap, nl, 4), dtype=torch.float32, device=dev)

    def _sync(self):
        """The grid's tensors as they are now against the state: another shape is an error, another tensor of the same shape
        (an assignment to the grid) becomes the foreground trainer's too. Returns the grid's handle."""
        g, fg = self.grid, self._fg.grid
        if tuple(g.background_data.shape) != tuple(self.grad_background.shape):
            raise ValueError(f"background_data changed shape since this trainer was made: {tuple(g.background_data.shape)}, "
                             f"gradients {tuple(self.grad_background.shape)}")
        if tuple(g.density_data.shape) != tuple(self.grad_density.shape) or tuple(g.sh_data.shape) != tuple(self.grad_sh.shape):
            raise ValueError(f"the grid's tables changed shape since this trainer was made: density_data "
                             f"{tuple(g.density_data.shape)}, sh_data {tuple(g.sh_data.shape)}; gradients "
                             f"{tuple(self.grad_density.shape)}, {tuple(self.grad_sh.shape)}")
        if fg.links is not g.links or fg.density_data is not g.density_data or fg.sh_data is not g.sh_data:
            fg.links, fg.density_data, fg.sh_data = g.links, g.density_data, g.sh_data
        return g._handle()      # validates all five tensors and re-attaches the background where it changed

    def zero_grad(self):
        """Zero the three gradients and the two masks (the kernels accumulate)."""
        self._fg.zero_grad()
        self.grad_background.zero_()
        self.mask_background.zero_()

    # ---- the step's parts -----------------------------------------------------------------------------------
    def forward_backward(self, rays: Rays, rgb_gt: torch.Tensor, return_log_transmit: bool = False):
        """Render ``rays`` (``rgb [N, 3]`` and the final ``log_transmit``, bit-identical to ``grid.volume_render(rays)``) and
        add the gradients of ``mean((rgb - rgb_gt) ** 2)`` to ``grad_density``, ``grad_sh`` and ``grad_background``, marking
        what was touched in ``mask`` and ``mask_background``. Five launches on one stream, no host wait: the taped foreground
        (brightness 0), the taped background pass, the foreground's backward from the combined tape, the background's."""
        return self._forward_backward(rays, rgb_gt, None, return_log_transmit)

    def volume_render_fused(self, rays: Rays, rgb_gt: torch.Tensor, randomize: bool = False, beta_loss: float = 0.0,
                            sparsity_loss: float = 0.0, return_log_transmit: bool = False):
        """svox2's ``grid.volume_render_fused`` with its two regularisers (``GridTrainer.volume_render_fused`` states them):
        the launches of :meth:`forward_backward`, with ``nerf_grid_render_backward_losses`` as the foreground's backward and
        the foreground's own ``log_transmit`` (before the background pass) as its ``T_in``, as in svox2. ``beta_loss`` is
        divided by the number of rays; ``sparsity_loss`` is passed as given and is applied to FOREGROUND samples only: svox2
        also applies it to the sigma samples of the background layers, which is not built
        (``nerf_grid_background_backward`` refuses it). ``grad_background`` does not depend on either weight.
        ``randomize=True`` is refused."""
        for name, v in (("beta_loss", beta_loss), ("sparsity_loss", sparsity_loss)):
            if not (math.isfinite(v) and v >= 0.0):
                raise ValueError(f"{name} = {v} must be finite and >= 0")
        if randomize:
            raise NotImplementedError("randomize is not built")
        return self._forward_backward(rays, rgb_gt, (float(beta_loss), float(sparsity_loss)), return_log_transmit)

    def _forward_backward(self, rays, rgb_gt, losses, return_log_transmit):
        """``losses``: ``None`` (the foreground's backward is ``nerf_grid_render_backward``) or ``(lambda_beta, sparsity_loss)``"""
        g = self.grid
        h = self._sync()
        opt = g.opt._to_c(False)
        fg_opt = g.opt._to_c(False)
        fg_opt.background_brightness = 0.0
        o = g._rays_arg(rays.origins, "rays.origins")
        d = g._rays_arg(rays.dirs, "rays.dirs", o.shape[0])
        n = o.shape[0]
        if not torch.is_tensor(rgb_gt):
            raise TypeError("rgb_gt must be a tensor")
        if not rgb_gt.is_cuda:
            raise RuntimeError("rgb_gt is on the CPU: BackgroundGrid has no CPU fallback")
        if rgb_gt.dim() != 2 or tuple(rgb_gt.shape) != (n, 3):
            raise ValueError(f"rgb_gt must be [{n}, 3] like the rays, got {tuple(rgb_gt.shape)}")
        dev, lib, stream = self.ctx.device, self.ctx.lib, self.ctx.stream().value
        gt = rgb_gt.detach().to(device=dev, dtype=torch.float32).contiguous()
        rgb = torch.empty((n, 3), device=dev, dtype=torch.float32)
        logt_fg = torch.empty((n,), device=dev, dtype=torch.float32)
        logt = torch.empty((n,), device=dev, dtype=torch.float32)
        tape = torch.empty((n, 3), device=dev, dtype=torch.float64)
        tape_bg = torch.empty((n, 3), device=dev, dtype=torch.float64)
        if n == 0:
            return (rgb, logt) if return_log_transmit else rgb
        a = GridRenderTapedArgs()
        a.origins, a.dirs, a.n_rays = o.data_ptr(), d.data_ptr(), n
        a.rgb_out, a.log_transmit, a.tape, a.use_skip, a.stream = rgb.data_ptr(), logt_fg.data_ptr(), tape.data_ptr(), 1, stream
        check(lib.nerf_grid_render_rays_taped(h, C.byref(fg_opt), C.byref(a)))
        b = GridBackgroundTapedArgs()
        b.origins, b.dirs, b.n_rays, b.rgb = o.data_ptr(), d.data_ptr(), n, rgb.data_ptr()
        b.log_transmit, b.log_transmit_out = logt_fg.data_ptr(), logt.data_ptr()
        b.tape, b.tape_background, b.stream = tape.data_ptr(), tape_bg.data_ptr(), stream
        check(lib.nerf_grid_background_rays_taped(h, C.byref(opt), C.byref(b)))
        # d loss / d rgb as nerf_grid_fused_backward forms it: (rgb - gt) * (2 / (3 n)), the factor an fp32 value
        scale = float(np.float32(2.0) / (np.float32(3.0) * np.float32(n)))
        grad_rgb = ((rgb - gt) * scale).contiguous()
        r = GridRenderBackwardArgs()
        r.origins, r.dirs, r.n_rays, r.grad_rgb, r.tape = o.data_ptr(), d.data_ptr(), n, grad_rgb.data_ptr(), tape.data_ptr()
        r.grad_density, r.grad_sh, r.mask = self.grad_density.data_ptr(), self.grad_sh.data_ptr(), self.mask.data_ptr()
        r.use_skip, r.stream = 1, stream
        if losses is None:
            check(lib.nerf_grid_render_backward(h, C.byref(fg_opt), C.byref(r)))
        else:
            ls = GridRenderBackwardLossesArgs()
            ls.beta_loss, ls.sparsity_loss, ls.log_transmit = losses[0] / n, losses[1], logt_fg.data_ptr()
            check(lib.nerf_grid_render_backward_losses(h, C.byref(fg_opt), C.byref(r), C.byref(ls)))
        w = GridBackgroundBackwardArgs()
        w.origins, w.dirs, w.n_rays, w.grad_rgb = o.data_ptr(), d.data_ptr(), n, grad_rgb.data_ptr()
        w.log_transmit, w.tape_background = logt_fg.data_ptr(), tape_bg.data_ptr()
        w.grad_background, w.mask_background, w.stream = self.grad_background.data_ptr(), self.mask_background.data_ptr(), stream
        check(lib.nerf_grid_background_backward(h, C.byref(opt), C.byref(w)))
        return (rgb, logt) if return_log_transmit else rgb

    def add_tv_grad(self, target: str = "density", scaling: float = 1.0, scaling_density: float = None, sparse_frac: float = 0.01,
                    start: int = None, start_dim: int = 0, end_dim: int = None, ignore_edge: bool = False):
        """``"density"`` / ``"sh"``: ``GridTrainer.add_tv_grad`` on the foreground tables (``ignore_edge`` included). ``"background"``: svox2's
        ``inplace_tv_background_grad`` over ``max(1, int(sparse_frac * 2R R L))`` cells of the ``[2R, R, L]`` volume starting at
        cell ``start`` (C order, wrapping past the last; drawn from ``self.generator`` when ``None``), with ``scaling`` for the
        colours and ``scaling_density`` (default: ``scaling``) for sigma; the kernel receives each divided by the count.
        Returns ``(start, count)``."""
        h = self._sync()
        if target in ("density", "sh"):
            if scaling_density is not None:
                raise ValueError("scaling_density belongs to target 'background'")
            return self._fg.add_tv_grad(target, scaling, sparse_frac, start, start_dim, end_dim, ignore_edge)
        if target != "background":
            raise ValueError(f"target {target!r}: 'density', 'sh' or 'background'")
        if ignore_edge:
            raise ValueError("ignore_edge belongs to the targets 'density' and 'sh'")
        if start_dim != 0 or end_dim is not None:
            raise ValueError("start_dim / end_dim belong to the targets 'density' and 'sh'")
        if not 0.0 < sparse_frac <= 1.0:
            raise ValueError(f"sparse_frac = {sparse_frac} must be in (0, 1]")
        g = self.grid
        n = g.background_links.numel() * g.background_data.shape[1]
        count = max(1, int(sparse_frac * n))
        if start is None:
            start = int(torch.randint(0, n, (1,), generator=self.generator).item())
        if not 0 <= start < n:
            raise ValueError(f"start = {start} outside [0, {n})")
        a = GridBackgroundTvArgs()
        a.start, a.count = start, count
        a.scale_color = float(scaling) / count
        a.scale_sigma = float(scaling if scaling_density is None else scaling_density) / count
        a.grad, a.mask, a.stream = self.grad_background.data_ptr(), self.mask_background.data_ptr(), self.ctx.stream().value
        check(self.ctx.lib.nerf_grid_background_tv_grad(h, C.byref(a)))
        return start, count

    def step(self, lr_sigma: float, lr_sh: float, lr_sigma_bg: float, lr_color_bg: float, beta: float = 0.95, epsilon: float = 1e-8,
             optim: str = "rmsprop", minval: float = -1e9):
        """One masked optimiser step on the three tables (svox2's ``optim_density_step``, ``optim_sh_step`` and
        ``optim_background_step``): entries whose mask byte is unset, and their ``rms``, are untouched. The gradients and the
        masks are left as they are."""
        self._sync()
        if optim not in ("rmsprop", "sgd"):
            raise ValueError(f"optim {optim!r}: 'rmsprop' or 'sgd'")
        self._fg.step(lr_sigma, lr_sh, beta, epsilon, optim, minval)
        data = self.grid.background_data
        a = GridBackgroundOptimArgs()
        a.data, a.rms, a.grad, a.mask = (data.data_ptr(), self.background_rms.data_ptr(), self.grad_background.data_ptr(),
                                         self.mask_background.data_ptr())
        a.rows = data.shape[0] * data.shape[1]
        a.kind = NERF_GRID_OPTIM_RMSPROP if optim == "rmsprop" else NERF_GRID_OPTIM_SGD
        a.beta, a.lr_sigma, a.lr_color, a.eps, a.minval = beta, lr_sigma_bg, lr_color_bg, epsilon, minval
        a.stream = self.ctx.stream().value
        check(self.ctx.lib.nerf_grid_background_optim_step(self.ctx.handle, C.byref(a)))

    def train_step(self, rays: Rays, rgb_gt: torch.Tensor, lr_sigma: float = 30.0, lr_sh: float = 1e-2, lr_sigma_bg: float = 3.0,
                   lr_color_bg: float = 0.1, beta: float = 0.95, epsilon: float = 1e-8, optim: str = "rmsprop",
                   lambda_tv: float = 0.0, lambda_tv_sh: float = 0.0, lambda_tv_background_sigma: float = 0.0,
                   lambda_tv_background_color: float = 0.0, tv_sparsity: float = 0.01, tv_background_sparsity: float = 0.01,
                   lambda_beta: float = 0.0, lambda_sparsity: float = 0.0, tv_sh_ignore_edge: bool = False):
        """``zero_grad``, ``forward_backward`` (``volume_render_fused`` where ``lambda_beta`` or ``lambda_sparsity`` is not
        zero), the TV gradients whose weight is not zero, ``step``. ``tv_sh_ignore_edge=True`` is what svox2's colour TV does.
        Returns ``{"mse", "psnr"}`` of the batch before the step (reading them waits for the device)."""
        self.zero_grad()
        if lambda_beta or lambda_sparsity:
            rgb = self.volume_render_fused(rays, rgb_gt, beta_loss=lambda_beta, sparsity_loss=lambda_sparsity)
        else:
            rgb = self.forward_backward(rays, rgb_gt)
        if lambda_tv:
            self.add_tv_grad("density", lambda_tv, sparse_frac=tv_sparsity)
        if lambda_tv_sh:
            self.add_tv_grad("sh", lambda_tv_sh, sparse_frac=tv_sparsity, ignore_edge=tv_sh_ignore_edge)
        if lambda_tv_background_sigma or lambda_tv_background_color:
            self.add_tv_grad("background", lambda_tv_background_color, lambda_tv_background_sigma, tv_background_sparsity)
        self.step(lr_sigma, lr_sh, lr_sigma_bg, lr_color_bg, beta, epsilon, optim)
        gt = rgb_gt.detach().to(device=rgb.device, dtype=torch.float32)
        mse = float(((rgb - gt) ** 2).mean()) if rgb.numel() else float("nan")
        return {"mse": mse, "psnr": -10.0 * math.log10(mse) if mse > 0 else float("inf")}

    # ---- changes of shape -----------------------------------------------------------------------------------
    def sparsify_background(self, sigma_thresh: float = 1.0, dilate: int = 1):
        """``grid.sparsify_background`` inside a training loop: the background's gradient, mask and RMSProp state are allocated
        anew at the kept rows and zeroed; the foreground, its state and its skip data are not touched. Returns the number of
        kept rows. An argument error leaves the grid and the trainer as they were."""
        self._sync()
        kept = self.grid.sparsify_background(sigma_thresh, dilate)
        self._allocate_background()
        return kept

    def _adopt_foreground(self, accelerate: bool):
        g, fg = self.grid, self._fg.grid
        g.links, g.density_data, g.sh_data = fg.links, fg.density_data, fg.sh_data
        if accelerate:
            g.accelerate()
        else:
            g._handle()

    def resample(self, reso, sigma_thresh: float = 5.0, weight_thresh: float = 0.01, dilate: int = 2, cameras=None,
                 accelerate: bool = True, weight_render_stop_thresh: float = 0.2, max_elements: int = 0):
        """``GridTrainer.resample`` of the foreground: ``links``, ``density_data`` and ``sh_data`` of the grid are replaced in
        place and the foreground's gradients, mask and RMSProp state are allocated anew and zeroed; the background, its state
        and its attachment are left alone (a new handle gets the background attached again). An argument error leaves the
        grid and the trainer as they were."""
        self._sync()
        self._fg.resample(reso, sigma_thresh, weight_thresh, dilate, cameras, False, weight_render_stop_thresh, max_elements)
        self._adopt_foreground(accelerate)

    def remove_floaters(self, accelerate: bool = True, **fdr_kwargs):
        """``GridTrainer.remove_floaters`` of the foreground, with the contract of :meth:`resample`. Returns the
        ``compute_FDR`` result of the foreground as it was."""
        self._sync()
        result = self._fg.remove_floaters(False, **fdr_kwargs)
        self._adopt_foreground(accelerate)
        return result
