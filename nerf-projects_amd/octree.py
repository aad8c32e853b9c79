"""PlenOctree: ``svox.N3Tree`` as a container, its ``.npz`` file (also ``compression.py``'s output), the build of a tree from
a sparse voxel grid (what svox2's ``to_svox1`` computes) and the renderer (``svox.VolumeRenderer.render_persp``), in HIP.

The container (fields, file, checks) works on any device with torch ops; building and rendering run in the kernels of
csrc/octree_kernels.hip, the gradient with respect to ``data`` (``loss.backward()`` through a render, and the fused
:meth:`N3Tree.mse_backward` that ``octree_optimize.optimize`` - ``plenoctree/octree/optimization.py``'s loop - steps with) in
csrc/octree_grad_kernels.hip; as everywhere in this package they have no CPU or PyTorch fallback. The arithmetic of the march is
defined in include/nerf_mi355x.h, "PlenOctree": svox itself is not part of the reference (it only calls into it), so what is
said here about svox's arrays, defaults and march is restated from memory of svox 0.2 and not verified against it; the array
names of the file are confirmed by the list ``plenoctree/octree/compression.py`` deletes, the channel order by
``compressed_evaluation.py``.
"""
import ctypes as C
import warnings
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import OctreeBackwardArgs, OctreeBuildArgs, OctreeDesc, OctreeRenderArgs, OctreeRenderOptions, check
from .grid import Camera, Rays, _refuse_half
from .host import get_context

__all__ = ["N3Tree", "DATA_FORMATS", "MAX_DEPTH"]

DATA_FORMATS = {"SH1": 1, "SH4": 4, "SH9": 9, "SH16": 16, "SH25": 25}
MAX_DEPTH = _lib.NERF_OCTREE_MAX_DEPTH
_ACTIVATIONS = {"sigmoid": _lib.NERF_OCTREE_RGB_SIGMOID, "relu_half": _lib.NERF_OCTREE_RGB_RELU_HALF}
# svox's names, in the order it writes them (compression.py:141-149 deletes five of them by name)
FILE_KEYS = ("data_dim", "child", "parent_depth", "n_internal", "n_free", "invradius3", "offset", "depth_limit",
             "geom_resize_fact", "data", "data_format")


def _basis_of(data_format):
    fmt = str(data_format)
    if fmt in DATA_FORMATS:
        return DATA_FORMATS[fmt]
    kind = fmt.rstrip("0123456789")
    if kind in ("RGBA", "SG", "ASG"):
        raise NotImplementedError(f"data_format {fmt!r}: only spherical harmonics (SH1, SH4, SH9, SH16, SH25) are built, not "
                                  f"{'plain RGBA' if kind == 'RGBA' else 'spherical Gaussians (' + kind + ')'}")
    raise ValueError(f"data_format {fmt!r} is none of {sorted(DATA_FORMATS)}")


def _three_floats(v, name):
    a = np.atleast_1d(np.asarray(v.detach().cpu() if torch.is_tensor(v) else v, dtype=np.float32)).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, 3)
    if a.size != 3:
        raise ValueError(f"{name}: expected a scalar or three values, got {v!r}")
    return torch.from_numpy(np.ascontiguousarray(a))


def measure_depth(child):
    """The checks a foreign ``child`` ``[n, 2, 2, 2]`` must pass before a kernel may walk it, with torch ops on its device;
    returns ``max_depth``, the depth of the deepest node (root: 0). ``ValueError`` for an entry that is negative or points
    at or past ``n`` (every other entry makes the index strictly increase, so every descent ends) and for a tree in which a
    level-by-level sweep from the root still finds nodes after ``MAX_DEPTH`` rounds."""
    n = child.shape[0]
    flat = child.reshape(n, 8).to(torch.int64)
    node = torch.arange(n, device=child.device).unsqueeze(1)
    if bool((flat < 0).any()):
        raise ValueError("child holds a negative entry")
    if bool(((flat > 0) & (node + flat >= n)).any()):
        raise ValueError(f"child holds an entry that points past the last of the {n} nodes")
    frontier = torch.zeros(1, dtype=torch.int64, device=child.device)
    depth = 0
    while True:
        step = flat[frontier]
        nxt = torch.unique((frontier.unsqueeze(1) + step)[step > 0])      # (unique: a file's graph need not be a tree)
        if nxt.numel() == 0:
            return depth
        if depth == MAX_DEPTH:
            raise ValueError(f"the tree is deeper than {MAX_DEPTH} levels")
        depth += 1
        frontier = nxt


class N3Tree:
    """``svox.N3Tree`` with branching factor 2. ``child`` int32 ``[n, 2, 2, 2]`` (0: leaf, else child index minus own index),
    ``data`` fp32 ``[n, 2, 2, 2, 3 B + 1]`` (a row is ``[R coefficients, G, B, sigma]``), ``parent_depth`` int32 ``[n, 2]``
    (flat index of the parent cell, depth), ``invradius`` / ``offset`` fp32 ``[3]`` on the host (world to unit cube:
    ``x * invradius + offset``), ``data_format`` ``"SH1" | "SH4" | "SH9" | "SH16" | "SH25"``, ``rgb_activation``
    ``"sigmoid"`` (svox) or ``"relu_half"`` (``max(0.5 + sum, 0)``: the colour model of a grid, see :meth:`from_grid`).
    ``max_depth`` is measured at construction (:func:`measure_depth`); the kernels bound every descent by it. Writing into
    ``child`` afterwards is not supported: make a new tree.
    ``data`` is the tree's one parameter (:meth:`parameters`, :meth:`requires_grad_`): once it requires grad, the renders
    are differentiable with respect to it, and :meth:`mse_backward` is the fused clamped-MSE step of ``optimization.py``.
    An optimizer must update ``data`` in place (torch's do): the kernels keep its address. Not built: gradients with respect
    to rays, editing (``refine``, ``shrink_to_fit``, ``merge``), fp16 ``data``, NDC, ``extra_data``."""

    def __init__(self, child, data, parent_depth=None, invradius=0.5, offset=0.5, data_format="SH9", rgb_activation="sigmoid",
                 N=2, extra_data=None, ndc=None, depth_limit=10, geom_resize_fact=1.0, device=None, _max_depth=None):
        if N != 2:
            raise NotImplementedError(f"N = {N}: only octrees (branching factor N = 2) are built")
        if extra_data is not None:
            raise NotImplementedError("extra_data is not built")
        if ndc is not None:
            raise NotImplementedError("NDC trees are not built")
        self.data_format = str(data_format)
        self.basis_dim = _basis_of(data_format)
        if rgb_activation not in _ACTIVATIONS:
            raise ValueError(f"rgb_activation {rgb_activation!r} is neither 'sigmoid' nor 'relu_half'")
        self.rgb_activation = rgb_activation
        child, data = torch.as_tensor(child), torch.as_tensor(data)
        dev = torch.device(device) if device is not None else child.device
        child = child.to(device=dev, dtype=torch.int32).contiguous()
        data = data.to(device=dev, dtype=torch.float32).contiguous()
        n = child.shape[0]
        if child.dim() != 4 or tuple(child.shape[1:]) != (2, 2, 2) or n < 1:
            raise ValueError(f"child must be [n, 2, 2, 2] with n >= 1, got {tuple(child.shape)}")
        if tuple(data.shape) != (n, 2, 2, 2, 3 * self.basis_dim + 1):
            raise ValueError(f"data must be [{n}, 2, 2, 2, {3 * self.basis_dim + 1}] for {self.data_format}, got {tuple(data.shape)}")
        if n > (1 << 27):
            raise ValueError(f"{n} nodes: at most 2^27")
        if parent_depth is None:
            parent_depth = torch.zeros((n, 2), dtype=torch.int32)
        parent_depth = torch.as_tensor(parent_depth).to(device=dev, dtype=torch.int32).contiguous()
        if tuple(parent_depth.shape) != (n, 2):
            raise ValueError(f"parent_depth must be [{n}, 2], got {tuple(parent_depth.shape)}")
        self.invradius = _three_floats(invradius, "invradius")
        self.offset = _three_floats(offset, "offset")
        if not bool((torch.isfinite(self.invradius) & (self.invradius > 0)).all()) or not bool(torch.isfinite(self.offset).all()):
            raise ValueError(f"invradius = {self.invradius.tolist()} must be positive and finite, offset = {self.offset.tolist()} finite")
        # (_max_depth: from_grid knows the depth of the tree its kernels wrote, and skips the sweep and its waits)
        self.max_depth = measure_depth(child) if _max_depth is None else int(_max_depth)
        self.child, self.data, self.parent_depth = child, data, parent_depth
        self.depth_limit, self.geom_resize_fact = int(depth_limit), float(geom_resize_fact)
        self._handle_ptr = None
        self._ctx = None
        self._capped = None

    # ---- svox's surface ---------------------------------------------------------------------------------
    N = 2

    @property
    def data_dim(self):
        return 3 * self.basis_dim + 1

    @property
    def n_internal(self):
        return int(self.child.shape[0])

    @property
    def n_leaves(self):
        return int((self.child == 0).sum())

    @property
    def device(self):
        return self.child.device

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.child, self.data, self.parent_depth))

    def to(self, device):
        """A tree with the same arrays on ``device`` (no check is repeated: the arrays are this tree's)."""
        t = object.__new__(N3Tree)
        t.__dict__.update(self.__dict__)
        t.child, t.data, t.parent_depth = (x.to(device) for x in (self.child, self.data, self.parent_depth))
        t._handle_ptr = t._ctx = t._capped = None
        return t

    def clone(self, device=None):
        """A tree with copies of the arrays (on ``device``, default: this tree's), detached from any graph; ``data`` requires
        grad where this tree's does. What ``optimization.py`` keeps as its best tree."""
        dev = self.device if device is None else torch.device(device)
        t = object.__new__(N3Tree)
        t.__dict__.update(self.__dict__)
        t.child, t.data, t.parent_depth = (x.detach().to(dev, copy=True) for x in (self.child, self.data, self.parent_depth))
        t.data.requires_grad_(self.data.requires_grad)
        t.invradius, t.offset = self.invradius.clone(), self.offset.clone()
        t._handle_ptr = t._ctx = t._capped = None
        return t

    def parameters(self):
        """``[data]``: ``torch.optim.SGD(tree.parameters(), lr=1e7)`` as in ``optimization.py``."""
        return [self.data]

    def requires_grad_(self, flag=True):
        self.data.requires_grad_(bool(flag))
        return self

    def _not_built(name, what):      # noqa: N805
        def f(self, *a, **k):
            raise NotImplementedError(f"N3Tree.{name}: {what} is not built")
        f.__name__ = name
        return f

    refine = _not_built("refine", "editing a tree (refine)")
    shrink_to_fit = _not_built("shrink_to_fit", "editing a tree (shrink_to_fit)")
    merge = _not_built("merge", "editing a tree (merge)")
    del _not_built

    # ---- the file -----------------------------------------------------------------------------------------
    def save(self, path, compress=False):
        """svox's ``.npz``: ``data_dim, child, parent_depth, n_internal, n_free, invradius3, offset, depth_limit,
        geom_resize_fact, data`` (fp16) and ``data_format``; and ``rgb_activation``, this package's one extra key."""
        z = {
            "data_dim": np.int64(self.data_dim),
            "child": self.child.cpu().numpy(),
            "parent_depth": self.parent_depth.cpu().numpy(),
            "n_internal": np.int64(self.n_internal),
            "n_free": np.int64(0),
            "invradius3": self.invradius.numpy(),
            "offset": self.offset.numpy(),
            "depth_limit": np.int64(self.depth_limit),
            "geom_resize_fact": np.float64(self.geom_resize_fact),
            "data": self.data.detach().cpu().numpy().astype(np.float16),
            "data_format": self.data_format,
            "rgb_activation": self.rgb_activation,
        }
        (np.savez_compressed if compress else np.savez)(path, **z)

    @classmethod
    def load(cls, path, device="cuda"):
        """A tree from svox's ``.npz`` or from a ``compression.py`` output of one (``quant_colors [Q, K, 3]``, ``quant_map
        [Q, n, 2, 2, 2]``, ``sigma [n, 2, 2, 2]`` and the optional ``data_retained [retain, n, 2, 2, 2, 3]``): coefficient
        ``retain + q`` of channel ``c`` is ``quant_colors[q, quant_map[q], c]`` (an index past the palette gives 0), the rule
        of ``compressed_evaluation.py``, applied with torch ops on ``device`` and rounded to fp16 as it does. ``child`` is
        checked (:func:`measure_depth`); a tree that fails is refused with ``ValueError``."""
        dev = torch.device(device)
        z = np.load(path)
        files = set(z.files)
        if "extra_data" in files and z["extra_data"].size:
            raise NotImplementedError("extra_data is not built")
        if "ndc_width" in files or "ndc" in files:
            raise NotImplementedError("NDC trees are not built")
        for keys in (("invradius3", "invradius"), ("offset",), ("child",)) + (() if "quant_colors" in files else (("data",),)):
            if not files & set(keys):
                raise ValueError(f"{path}: no array named {' or '.join(keys)}: not an N3Tree file")
        child = np.asarray(z["child"])
        if child.ndim != 4 or child.shape[1:] != (2, 2, 2):
            if child.ndim == 4 and child.shape[1] == child.shape[2] == child.shape[3]:
                raise NotImplementedError(f"N = {child.shape[1]}: only octrees (branching factor N = 2) are built")
            raise ValueError(f"child must be [n, 2, 2, 2], got {child.shape}")
        child_t = torch.from_numpy(np.ascontiguousarray(child.astype(np.int32))).to(dev)
        fmt = str(z["data_format"].item() if hasattr(z["data_format"], "item") else z["data_format"]) if "data_format" in files else None
        if "quant_colors" in files:
            colors = torch.from_numpy(np.asarray(z["quant_colors"]).astype(np.float32)).to(dev)            # [Q, K, 3]
            qmap = torch.from_numpy(np.asarray(z["quant_map"]).astype(np.int64)).to(dev)                   # [Q, n, 2, 2, 2]
            sigma = torch.from_numpy(np.asarray(z["sigma"]).astype(np.float32)).to(dev)
            parts = []
            if "data_retained" in files:
                parts.append(torch.from_numpy(np.asarray(z["data_retained"]).astype(np.float32)).to(dev))  # [retain, n, 2, 2, 2, 3]
            valid = (qmap < colors.shape[1]).unsqueeze(-1)
            idx = qmap.clamp(max=colors.shape[1] - 1)
            looked = torch.stack([colors[q][idx[q]] for q in range(colors.shape[0])], 0)                  # [Q, n, 2, 2, 2, 3]
            parts.append(torch.where(valid, looked, torch.zeros_like(looked)))
            coeff = torch.cat(parts, 0)                                                                    # [B, n, 2, 2, 2, 3]
            B = coeff.shape[0]
            rgb = coeff.permute(1, 2, 3, 4, 5, 0).reshape(coeff.shape[1], 2, 2, 2, 3 * B)                  # channel-major
            data = torch.cat([rgb, sigma.unsqueeze(-1)], -1).to(torch.float16).to(torch.float32)
            if fmt is None:
                fmt = f"SH{B}"
        else:
            data = torch.from_numpy(np.asarray(z["data"]).astype(np.float32)).to(dev)
            if fmt is None:
                fmt = f"SH{(data.shape[-1] - 1) // 3}"
        invradius = z["invradius3"] if "invradius3" in files else z["invradius"]
        act = str(z["rgb_activation"].item() if hasattr(z["rgb_activation"], "item") else z["rgb_activation"]) if "rgb_activation" in files else "sigmoid"
        pd = torch.from_numpy(np.asarray(z["parent_depth"]).astype(np.int32)) if "parent_depth" in files else None
        return cls(child_t, data, pd, invradius, z["offset"], fmt, act, device=dev,
                   depth_limit=int(z["depth_limit"]) if "depth_limit" in files else 10,
                   geom_resize_fact=float(z["geom_resize_fact"]) if "geom_resize_fact" in files else 1.0)

    # ---- from a grid --------------------------------------------------------------------------------------
    @classmethod
    def from_grid(cls, grid):
        """svox2's ``SparseGrid.to_svox1`` on the GPU (csrc/octree_kernels.hip): a cubic grid of side ``R = 2^L`` becomes the
        tree whose leaf cell ``(i, j, k)`` at depth ``L`` holds ``[sh_data row, density]`` of lattice node ``(i, j, k)`` where
        ``links >= 0`` and zeros elsewhere; empty regions are zero leaves at the shallowest level, nodes are numbered breadth
        first (two builds give the same bits). ``rgb_activation`` is ``"relu_half"``, so that the tree's leaf colours are the
        grid's node colours; svox would silently render them through a sigmoid. One wait, for the node count (``max_depth`` is
        known from ``R``, so the container's sweep is not run).
        ``SparseGrid.to_svox1`` itself keeps raising, as the other svox2-named methods of ``SparseGrid`` do: this is the name."""
        _refuse_half(grid, "N3Tree.from_grid")
        reso = list(grid.links.shape)
        R = reso[0]
        if reso != [R, R, R] or R < 2 or R & (R - 1):
            raise ValueError(f"N3Tree.from_grid: the grid is {reso}: an octree needs a cube whose side is a power of two >= 2")
        ctx = grid.ctx
        h = grid._handle()
        ws_bytes = int(ctx.lib.nerf_octree_build_workspace(R))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=ctx.device)
        n_nodes = C.c_int64(0)
        a = OctreeBuildArgs()
        a.workspace, a.workspace_bytes, a.n_nodes = ws.data_ptr(), ws_bytes, C.pointer(n_nodes)
        a.stream = ctx.stream().value
        check(ctx.lib.nerf_octree_build_from_grid(h, C.byref(a)))
        n = int(n_nodes.value)
        D = 3 * grid.basis_dim + 1
        child = torch.empty((n, 2, 2, 2), dtype=torch.int32, device=ctx.device)
        parent_depth = torch.empty((n, 2), dtype=torch.int32, device=ctx.device)
        data = torch.empty((n, 2, 2, 2, D), dtype=torch.float32, device=ctx.device)
        a.child, a.parent_depth, a.data = child.data_ptr(), parent_depth.data_ptr(), data.data_ptr()
        check(ctx.lib.nerf_octree_build_from_grid(h, C.byref(a)))
        radius, center = grid.radius, grid.center      # fp32, host
        L = R.bit_length() - 1      # nodes of every depth 1 .. L - 1 exist as soon as one node is kept
        return cls(child, data, parent_depth, 0.5 / radius, 0.5 * (1.0 - center / radius), f"SH{grid.basis_dim}", "relu_half",
                   _max_depth=L - 1 if n > 1 else 0)

    # ---- rendering ----------------------------------------------------------------------------------------
    def _drop_handle(self):
        if getattr(self, "_handle_ptr", None) is not None:
            try:
                self._ctx.lib.nerf_octree_destroy(self._handle_ptr)
            except Exception:      # (interpreter shutdown)
                pass
        self._handle_ptr = None

    __del__ = _drop_handle

    def _handle(self):
        if self._handle_ptr is not None:
            return self._handle_ptr
        if not self.child.is_cuda:
            raise RuntimeError(f"the tree is on {self.child.device}: rendering has no CPU fallback (tree.to('cuda'))")
        ctx = get_context(self.child.device)
        d = OctreeDesc()
        d.n_nodes, d.data_dim, d.max_depth = self.child.shape[0], self.data_dim, self.max_depth
        d.rgb_activation = _ACTIVATIONS[self.rgb_activation]
        d.invradius[:] = self.invradius.tolist()
        d.offset[:] = self.offset.tolist()
        d.child, d.data, d.stream = self.child.data_ptr(), self.data.data_ptr(), ctx.stream().value
        h = C.c_void_p()
        check(ctx.lib.nerf_octree_create(ctx.handle, C.byref(d), C.byref(h)))
        self._ctx, self._handle_ptr = ctx, h
        self._capped = torch.zeros(1, dtype=torch.int64, device=ctx.device)
        self._capped_host = torch.zeros(1, dtype=torch.int64).pin_memory()
        self._capped_seen = 0
        return h

    def accelerate(self, levels=6):
        """A dense table of side ``2^k``, ``k = min(levels, max_depth)``, built by one kernel: every later descent starts at
        the table's cell for its position instead of the root. An accelerated render equals a plain one bit for bit, steps
        included (the header has the argument). ``levels=0`` drops the table. Returns ``k``."""
        levels = int(levels)
        if not 0 <= levels <= 8:
            raise ValueError(f"levels = {levels} must be in [0, 8]")
        h = self._handle()
        check(self._ctx.lib.nerf_octree_accelerate(h, levels, self._ctx.stream()))
        return self.table_levels

    @property
    def table_levels(self):
        """``k`` of the current table of :meth:`accelerate`, 0 without one."""
        return 0 if self._handle_ptr is None else int(self._ctx.lib.nerf_octree_table_levels(self._handle_ptr))

    def capped_rays(self):
        """Rays whose march ended at the cap of 65536 passes since the tree was made (waits for the device)."""
        return 0 if self._capped is None else int(self._capped.item())

    def _options(self, step_size, sigma_thresh, stop_thresh, background_brightness, fast):
        if fast:
            sigma_thresh = stop_thresh = 1e-2
        step_size = float(step_size)
        if not (step_size > 0.0 and np.isfinite(step_size)):
            raise ValueError(f"step_size = {step_size!r} must be positive and finite")
        o = OctreeRenderOptions()
        o.step_size, o.sigma_thresh, o.stop_thresh = step_size, float(sigma_thresh), float(stop_thresh)
        o.background_brightness = float(background_brightness)
        return o

    def _rays_arg(self, t, name, ctx, n=None):
        if not torch.is_tensor(t):
            raise TypeError(f"{name} must be a tensor")
        if not t.is_cuda:
            raise RuntimeError(f"{name} is on the CPU: the octree renderer has no CPU fallback")
        if t.requires_grad:
            raise NotImplementedError("gradients with respect to rays are not built: an N3Tree's parameter is its data")
        if t.dim() != 2 or t.shape[1] != 3 or (n is not None and t.shape[0] != n):
            raise ValueError(f"{name} must be [N, 3], got {tuple(t.shape)}")
        return t.detach().to(device=ctx.device, dtype=torch.float32).contiguous()

    def _warn_capped(self, stacklevel):
        # the cap's counter as the previous call's copy left it on the host: reported without a wait
        seen = int(self._capped_host.item())
        if seen > self._capped_seen:
            warnings.warn(f"{seen - self._capped_seen} rays ended at the cap of 65536 march passes", RuntimeWarning, stacklevel=stacklevel + 1)
            self._capped_seen = seen

    @staticmethod
    def _refuse_ray_grads(rays):
        # (before anything needs a device: the refusal is the same on every tree)
        for x in (rays.origins, rays.dirs):
            if torch.is_tensor(x) and x.requires_grad:
                raise NotImplementedError("gradients with respect to rays are not built: an N3Tree's parameter is its data")

    def _render(self, cam, rays, opt, return_steps):
        if cam is None:
            self._refuse_ray_grads(rays)
        self._handle()
        ctx = self._ctx
        self._warn_capped(3)
        o = d = None
        if cam is None:
            o = self._rays_arg(rays.origins, "rays.origins", ctx)
            d = self._rays_arg(rays.dirs, "rays.dirs", ctx, o.shape[0])
        if self.data.requires_grad and torch.is_grad_enabled():
            out = _RenderFunction.apply(self.data, self, cam, o, d, opt, return_steps)
            return out if return_steps else out[0]
        return self._launch_render(cam, o, d, opt, return_steps)

    def _launch_render(self, cam, o, d, opt, return_steps):
        h, ctx = self._handle_ptr, self._ctx
        a = OctreeRenderArgs()
        if cam is not None:
            c = cam._to_c()
            n = cam.width * cam.height
        else:
            n = o.shape[0]
            a.origins, a.dirs, a.n_rays = o.data_ptr(), d.data_ptr(), n
        rgb = torch.empty((n, 3), device=ctx.device, dtype=torch.float32)
        steps = torch.empty((n,), device=ctx.device, dtype=torch.int32) if return_steps else None
        a.rgb = rgb.data_ptr()
        a.steps = 0 if steps is None else steps.data_ptr()
        a.capped = self._capped.data_ptr()
        a.stream = ctx.stream().value
        if cam is not None:
            check(ctx.lib.nerf_octree_render_image(h, C.byref(c), C.byref(opt), C.byref(a)))
        else:
            check(ctx.lib.nerf_octree_render_rays(h, C.byref(opt), C.byref(a)))
        self._capped_host.copy_(self._capped, non_blocking=True)
        return (rgb, steps) if return_steps else rgb

    def _launch_backward(self, cam, o, d, opt, grad_data, grad_rgb=None, rgb_gt=None, loss_scale=0.0, loss=None, rgb=None):
        """One launch of csrc/octree_grad_kernels.hip: adds into ``grad_data``; every array is a checked device tensor."""
        h, ctx = self._handle_ptr, self._ctx
        a = OctreeBackwardArgs()
        if cam is None:
            a.origins, a.dirs, a.n_rays = o.data_ptr(), d.data_ptr(), o.shape[0]
        a.grad_rgb = 0 if grad_rgb is None else grad_rgb.data_ptr()
        a.rgb_gt = 0 if rgb_gt is None else rgb_gt.data_ptr()
        a.loss_scale = float(loss_scale)
        a.grad_data = grad_data.data_ptr()
        a.loss = 0 if loss is None else loss.data_ptr()
        a.rgb = 0 if rgb is None else rgb.data_ptr()
        a.capped = self._capped.data_ptr()
        a.stream = ctx.stream().value
        if cam is not None:
            c = cam._to_c()
            check(ctx.lib.nerf_octree_backward_image(h, C.byref(c), C.byref(opt), C.byref(a)))
        else:
            check(ctx.lib.nerf_octree_backward_rays(h, C.byref(opt), C.byref(a)))
        self._capped_host.copy_(self._capped, non_blocking=True)

    def mse_backward(self, camera_or_rays, rgb_gt, step_size=1e-3, sigma_thresh=0.0, stop_thresh=0.0, background_brightness=1.0,
                     fast=False):
        """``mse = ((render.clamp(0, 1) - rgb_gt) ** 2).mean(); mse.backward()`` in one launch: renders ``camera_or_rays`` (a
        :class:`Camera` or :class:`Rays`), adds the gradient of ``mse`` into ``tree.data.grad`` (zeros are allocated where
        that is ``None``) and returns ``mse`` as a 0-dim device tensor, without a wait. ``rgb_gt``: ``[H, W, 3]`` or
        ``[N, 3]`` on the device. A NaN ray adds nothing to either (torch would give a NaN loss)."""
        opt = self._options(step_size, sigma_thresh, stop_thresh, background_brightness, fast)
        if not isinstance(camera_or_rays, Camera):
            self._refuse_ray_grads(camera_or_rays)
        self._handle()
        ctx = self._ctx
        self._warn_capped(2)
        cam = o = d = None
        if isinstance(camera_or_rays, Camera):
            cam = camera_or_rays
            n = cam.width * cam.height
        else:
            o = self._rays_arg(camera_or_rays.origins, "rays.origins", ctx)
            d = self._rays_arg(camera_or_rays.dirs, "rays.dirs", ctx, o.shape[0])
            n = o.shape[0]
        if not torch.is_tensor(rgb_gt) or not rgb_gt.is_cuda:
            raise RuntimeError("rgb_gt must be a tensor on the tree's device: the octree's backward has no CPU fallback")
        if rgb_gt.numel() != 3 * n or rgb_gt.shape[-1] != 3:
            raise ValueError(f"rgb_gt must hold [{n}, 3] colours, got {tuple(rgb_gt.shape)}")
        gt = rgb_gt.detach().to(device=ctx.device, dtype=torch.float32).reshape(n, 3).contiguous()
        if self.data.grad is None:
            self.data.grad = torch.zeros_like(self.data)
        loss = torch.zeros(1, device=ctx.device, dtype=torch.float32)
        if n:
            self._launch_backward(cam, o, d, opt, self.data.grad, rgb_gt=gt, loss_scale=2.0 / (3 * n), loss=loss)
        return loss[0] / max(3 * n, 1)

    def volume_render(self, rays: Rays, step_size=1e-3, sigma_thresh=0.0, stop_thresh=0.0, background_brightness=1.0,
                      fast=False, return_steps=False):
        """``[N, 3]`` colours of ``rays``; ``rays.dirs`` is used as given, as the march direction (any length) and as the
        argument of the SH basis (svox expects it normalised). Where ``tree.data`` requires grad and grad mode is on, the
        colours - the same bits - carry the gradient with respect to ``data`` (steps carry none); rays that require grad
        keep raising. ``step_size`` is svox's default as remembered (the
        reference's configs pass 1e-5); ``fast`` sets both thresholds to 1e-2. With ``return_steps`` also int32 ``[N]``, the
        leaves each ray visited."""
        return self._render(None, rays, self._options(step_size, sigma_thresh, stop_thresh, background_brightness, fast), return_steps)

    def volume_render_image(self, camera: Camera, step_size=1e-3, sigma_thresh=0.0, stop_thresh=0.0, background_brightness=1.0,
                            fast=False, return_steps=False):
        """``[H, W, 3]`` (and ``[H, W]`` steps): the rays of ``camera`` (OpenCV convention, unit directions) are made inside
        the launch; equal to :meth:`volume_render` on ``camera.gen_rays()`` bit for bit."""
        out = self._render(camera, None, self._options(step_size, sigma_thresh, stop_thresh, background_brightness, fast), return_steps)
        H, W = camera.height, camera.width
        return (out[0].view(H, W, 3), out[1].view(H, W)) if return_steps else out.view(H, W, 3)

    def render_persp(self, c2w, width=800, height=800, fx=1111.111, fy: Optional[float] = None, fast=False, **options):
        """``svox.VolumeRenderer(tree, **options).render_persp(c2w, ...)``: ``c2w`` in NeRF's OpenGL convention, ``[H, W, 3]``.
        A wrapper of :meth:`volume_render_image` on ``Camera.from_nerf_pose``."""
        cam = Camera.from_nerf_pose(c2w, height, width, fx)
        cam.fy = None if fy is None else float(fy)
        return self.volume_render_image(cam, fast=fast, **options)


class _RenderFunction(torch.autograd.Function):
    """A render whose backward is nerf_octree_backward_rays / _image: the colours are the plain render's bits."""

    @staticmethod
    def forward(ctx, data, tree, cam, o, d, opt, return_steps):
        out = tree._launch_render(cam, o, d, opt, return_steps)
        ctx.tree, ctx.cam, ctx.o, ctx.d, ctx.opt = tree, cam, o, d, opt
        if return_steps:
            ctx.mark_non_differentiable(out[1])
            return out
        return (out,)

    @staticmethod
    def backward(ctx, grad_rgb, *_):
        tree = ctx.tree
        grad = torch.zeros_like(tree.data)
        g = grad_rgb.detach().to(dtype=torch.float32).contiguous()
        if g.shape[0]:
            tree._launch_backward(ctx.cam, ctx.o, ctx.d, ctx.opt, grad, grad_rgb=g)
        return grad, None, None, None, None, None, None
