"""Sparse voxel grid (Plenoxels): render a scene from a lattice of densities and spherical-harmonic colours, no network.

``SparseGrid``, ``Rays``, ``Camera`` and ``RenderOptions`` carry the names, argument order and defaults of ``svox2`` for the
forward (inference) side: ``volume_render``, ``volume_render_image``, ``volume_render_depth``, ``volume_render_depth_image``,
``sample``, ``accelerate``, ``save`` / ``load`` in the ``.npz`` layout of Plenoxels checkpoints. ``SparseGrid.from_nerf`` bakes
one of this package's ``NeRF`` models into a grid.
The semantics of every call are stated in include/nerf_mi355x.h, "Sparse voxel grid"; everything runs in HIP kernels
(csrc/grid_kernels.hip, csrc/grid_depth_kernels.hip) and, as everywhere in this package, there is no CPU or PyTorch fallback.
What svox2 has and this module does not (learned bases, the other backends) raises ``NotImplementedError``, and so do background
layers on ``SparseGrid`` itself: a grid with them is ``grid_background.BackgroundGrid``. So do the svox2-named
training methods on ``SparseGrid`` - training a grid is ``grid_train.GridTrainer``, under names of its own.
``SparseGrid.to_half()`` gives the inference twin with fp16 colours on the device, ``grid_half.HalfGrid``.
"""
import ctypes as C
from dataclasses import dataclass, replace
from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._lib import (GridCamera, GridDepthArgs, GridProjectArgs, GridRaysToNdcArgs, GridRenderArgs, GridRenderOptions, GridSampleArgs, SparseGridDesc,
                   check)
from .host import NeRF, get_context, get_embedder, run_network
from .mesh import _axes, density_grid
from .occupancy import OccupancyGrid

__all__ = ["SparseGrid", "Rays", "Camera", "NdcCamera", "rays_to_ndc", "RenderOptions", "BASIS_TYPE_SH", "BASIS_TYPE_3D_TEXTURE", "BASIS_TYPE_MLP",
           "eval_sh_bases", "fibonacci_directions", "sh_projection_matrix"]

BASIS_TYPE_SH = 1
BASIS_TYPE_3D_TEXTURE = 4
BASIS_TYPE_MLP = 255

_SH_C0 = 0.28209479177387814
_SH_C1 = 0.4886025119029199
_SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)


def eval_sh_bases(basis_dim, dirs):
    """The real spherical-harmonic basis of degree <= 2 in svox2's sign and ordering convention at unit ``dirs`` ``[..., 3]``
    (numpy, in the dtype of ``dirs``): ``[..., basis_dim]``."""
    dirs = np.asarray(dirs)
    out = np.empty(dirs.shape[:-1] + (basis_dim,), dtype=dirs.dtype)
    c = dirs.dtype.type
    out[..., 0] = c(_SH_C0)
    if basis_dim > 1:
        x, y, z = dirs[..., 0], dirs[..., 1], dirs[..., 2]
        out[..., 1] = c(-_SH_C1) * y
        out[..., 2] = c(_SH_C1) * z
        out[..., 3] = c(-_SH_C1) * x
        if basis_dim > 4:
            xx, yy, zz = x * x, y * y, z * z
            out[..., 4] = c(_SH_C2[0]) * (x * y)
            out[..., 5] = c(_SH_C2[1]) * (y * z)
            out[..., 6] = c(_SH_C2[2]) * (c(2.0) * zz - xx - yy)
            out[..., 7] = c(_SH_C2[3]) * (x * z)
            out[..., 8] = c(_SH_C2[4]) * (xx - yy)
    return out


def fibonacci_directions(n):
    """``n`` unit directions of the spherical Fibonacci lattice, fp64 ``[n, 3]``: ``z_i = 1 - (2 i + 1) / n``, azimuth
    ``i * pi * (3 - sqrt(5))`` (the golden angle). Deterministic; nearly uniform, so the SH basis on it is nearly orthogonal."""
    i = np.arange(n, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / n
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], -1)


def sh_projection_matrix(basis_dim, n_dirs):
    """``(P, Y, dirs)`` in fp64: ``Y [n_dirs, basis_dim]`` the SH basis at ``fibonacci_directions(n_dirs)`` and
    ``P = pinv(Y) [basis_dim, n_dirs]``, the least-squares projection of samples on those directions (``P @ Y = I``)."""
    if n_dirs < basis_dim:
        raise ValueError(f"n_dirs = {n_dirs} directions cannot determine {basis_dim} SH coefficients")
    dirs = fibonacci_directions(n_dirs)
    Y = eval_sh_bases(basis_dim, dirs)
    return np.linalg.pinv(Y), Y, dirs


@dataclass
class RenderOptions:
    """svox2.RenderOptions. The forward cuvol kernel reads ``step_size`` (in voxels), ``sigma_thresh``, ``stop_thresh``,
    ``background_brightness`` and ``near_clip``; anything else must keep its default."""
    backend: str = "cuvol"
    background_brightness: float = 1.0
    step_size: float = 0.5
    sigma_thresh: float = 1e-10
    stop_thresh: float = 1e-7
    last_sample_opaque: bool = False
    near_clip: float = 0.0
    use_spheric_clip: bool = False
    random_sigma_std: float = 1.0
    random_sigma_std_background: float = 1.0

    def _to_c(self, randomize=False):
        if self.backend != "cuvol":
            raise NotImplementedError(f"backend {self.backend!r}: only the cuvol renderer is built (not svox1 / nvol)")
        if self.last_sample_opaque:
            raise NotImplementedError("last_sample_opaque is not built")
        if self.use_spheric_clip:
            raise NotImplementedError("use_spheric_clip is not built")
        if randomize:
            raise NotImplementedError("randomize (sigma noise) is not built")
        o = GridRenderOptions()
        o.step_size, o.sigma_thresh, o.stop_thresh = self.step_size, self.sigma_thresh, self.stop_thresh
        o.background_brightness, o.near_clip = self.background_brightness, self.near_clip
        return o


@dataclass
class Rays:
    origins: torch.Tensor
    dirs: torch.Tensor

    def __getitem__(self, key):
        return Rays(self.origins[key], self.dirs[key])

    @property
    def is_cuda(self) -> bool:
        return self.origins.is_cuda and self.dirs.is_cuda


@dataclass
class Camera:
    """svox2.Camera: ``c2w`` ``[3, 4]`` or ``[4, 4]`` in the OpenCV convention (x right, y down, z forward), pixel centres at
    ``+ 0.5``. This package's ``get_rays`` / ``synthetic.lego_camera`` use NeRF's OpenGL convention: :meth:`from_nerf_pose`."""
    c2w: torch.Tensor
    fx: float = 1111.11
    fy: Optional[float] = None
    cx: Optional[float] = None
    cy: Optional[float] = None
    width: int = 800
    height: int = 800
    ndc_coeffs: Union[Tuple[float, float], List[float]] = (-1.0, -1.0)

    @classmethod
    def from_nerf_pose(cls, c2w, H, W, focal):
        """The camera whose rays are those of ``get_rays(H, W, K, c2w)`` with ``K = [[focal, 0, W / 2], [0, focal, H / 2], ...]``:
        columns y and z of the rotation negated (OpenGL -> OpenCV), and ``cx = W / 2 + 0.5``, ``cy = H / 2 + 0.5`` because svox2
        looks through pixel centres ``x + 0.5`` where ``get_rays`` looks through ``x``."""
        m = torch.as_tensor(np.asarray(c2w.detach().cpu() if torch.is_tensor(c2w) else c2w), dtype=torch.float32)[:3, :4].clone()
        m[:, 1:3] *= -1.0
        return cls(m, fx=float(focal), cx=W * 0.5 + 0.5, cy=H * 0.5 + 0.5, width=int(W), height=int(H))

    @property
    def fx_val(self):
        return self.fx

    @property
    def fy_val(self):
        return self.fx if self.fy is None else self.fy

    @property
    def cx_val(self):
        return self.width * 0.5 if self.cx is None else self.cx

    @property
    def cy_val(self):
        return self.height * 0.5 if self.cy is None else self.cy

    @property
    def using_ndc(self):
        return self.ndc_coeffs[0] > 0.0

    @property
    def is_cuda(self) -> bool:
        return self.c2w.is_cuda

    def _to_c(self):
        if self.using_ndc:
            raise NotImplementedError("NDC cameras are not built into Camera: use NdcCamera")
        return self._pinhole_c()

    def _pinhole_c(self):
        c = GridCamera()
        m = torch.as_tensor(self.c2w).detach().to(device="cpu", dtype=torch.float32)
        if m.dim() != 2 or m.shape[0] < 3 or m.shape[1] != 4:
            raise ValueError(f"c2w must be [3, 4] or [4, 4], got {tuple(m.shape)}")
        c.c2w[:] = m[:3].reshape(-1).tolist()
        c.fx, c.fy, c.cx, c.cy = float(self.fx_val), float(self.fy_val), float(self.cx_val), float(self.cy_val)
        c.width, c.height = int(self.width), int(self.height)
        return c

    def gen_rays(self, device=None) -> Rays:
        """``Rays`` ``(origins [H * W, 3], dirs [H * W, 3])`` made on the GPU by the device function
        ``volume_render_image`` uses (fp64, rounded to fp32, as svox2's ``gen_rays``)."""
        c = self._to_c()
        ctx = get_context(device if device is not None else (self.c2w.device if self.is_cuda else None))
        n = self.width * self.height
        o = torch.empty((n, 3), device=ctx.device, dtype=torch.float32)
        d = torch.empty((n, 3), device=ctx.device, dtype=torch.float32)
        check(ctx.lib.nerf_grid_gen_rays(ctx.handle, C.byref(c), o.data_ptr(), d.data_ptr(), ctx.stream()))
        return Rays(o, d)


def _ndc_coeffs_arg(ndc_coeffs):
    try:
        vals = [float(v) for v in ndc_coeffs]
    except (TypeError, ValueError):
        raise ValueError(f"ndc_coeffs = {ndc_coeffs!r} must be two finite positive numbers") from None
    if len(vals) != 2 or not all(np.isfinite(v) and v > 0.0 for v in vals):
        raise ValueError(f"ndc_coeffs = {ndc_coeffs!r} must be two finite positive numbers")
    return vals


@dataclass
class NdcCamera(Camera):
    """A ``Camera`` of a forward-facing scene: svox2's ``Camera(..., ndc_coeffs=(2 fx / w, 2 fy / h))``. The same fields;
    ``ndc_coeffs`` must be two finite positive numbers. Every pixel's ray, made as ``Camera``'s and rounded to fp32, goes
    through ``rays_to_ndc`` on the device (svox2's ``convert_to_ndc`` and the normalisation after it, bit for bit), in
    ``gen_rays`` and inside every image kernel alike. ``Camera`` itself keeps refusing ``ndc_coeffs``: the capability has
    this name. The floater views and ``BackgroundGrid`` refuse it (they have no NDC form in svox2 either)."""

    def __post_init__(self):
        self.ndc_coeffs = tuple(_ndc_coeffs_arg(self.ndc_coeffs))

    def _to_c(self):
        c = self._pinhole_c()
        c.ndc_coeffs[:] = _ndc_coeffs_arg(self.ndc_coeffs)      # (checked again: a dataclass field can be reassigned)
        return c


def rays_to_ndc(rays: Rays, ndc_coeffs) -> Rays:
    """World rays -> the NDC rays svox2 trains and renders forward-facing scenes with: ``svox2.utils.convert_to_ndc`` with
    ``near = 1`` and ``dirs /= |dirs|``, one HIP launch, one lane per ray (the device function ``NdcCamera`` and the LLFF
    batches use; the sequence of operations is in include/nerf_mi355x.h). For callers who bring their own rays. A ray with
    ``dirs.z == 0`` comes back non-finite and renders as a miss."""
    coeffs = _ndc_coeffs_arg(ndc_coeffs)
    arrs = []
    for t, name in ((rays.origins, "rays.origins"), (rays.dirs, "rays.dirs")):
        if not torch.is_tensor(t):
            raise TypeError(f"{name} must be a tensor")
        if not t.is_cuda:
            raise RuntimeError(f"{name} is on the CPU: rays_to_ndc has no CPU fallback")
        if t.dim() != 2 or t.shape[1] != 3 or (arrs and t.shape[0] != arrs[0].shape[0]):
            raise ValueError(f"{name} must be [N, 3], got {tuple(t.shape)}")
        arrs.append(t.detach().to(dtype=torch.float32).contiguous())
    o, d = arrs
    if o.device != d.device:
        raise RuntimeError(f"rays.origins is on {o.device}, rays.dirs on {d.device}")
    n = o.shape[0]
    if n > (1 << 26):
        raise ValueError(f"{n} rays: at most 2^26 per call")
    ctx = get_context(o.device)
    oo, dd = torch.empty_like(o), torch.empty_like(d)
    a = GridRaysToNdcArgs()
    a.origins, a.dirs, a.n = o.data_ptr(), d.data_ptr(), n
    a.ndc_coeffs[:] = coeffs
    a.origins_out, a.dirs_out, a.stream = oo.data_ptr(), dd.data_ptr(), ctx.stream().value
    check(ctx.lib.nerf_grid_rays_to_ndc(ctx.handle, C.byref(a)))
    return Rays(oo, dd)


def _three(v, name):
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().tolist()
    vals = [float(x) for x in np.atleast_1d(np.asarray(v, dtype=np.float64)).tolist()]
    if len(vals) == 1:
        vals *= 3
    if len(vals) != 3:
        raise ValueError(f"{name}: expected a scalar or three values, got {v!r}")
    return torch.tensor(vals, dtype=torch.float32, device="cpu")


MAX_LATTICE = 1 << 30


def _reso3(reso, name="reso"):
    if isinstance(reso, (int, np.integer)) and not isinstance(reso, bool):
        reso = [int(reso)] * 3
    else:
        try:
            reso = [int(r) for r in reso]
        except TypeError:
            raise ValueError(f"{name} must be an integer or indexable object of 3 ints") from None
    if len(reso) != 3:
        raise ValueError(f"{name} must be an integer or indexable object of 3 ints")
    if any(r < 2 or r > 1024 for r in reso) or reso[0] * reso[1] * reso[2] > MAX_LATTICE:
        raise ValueError(f"{name} = {reso}: every side must be in [2, 1024] and the lattice hold at most 2^30 nodes")
    return reso


def _volume_arg(t, name, dtype, ctx=None):
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on the CPU: grid resampling has no CPU fallback")
    if ctx is not None and t.device != ctx.device:
        raise RuntimeError(f"{name} is on {t.device}, the grid on {ctx.device}")
    if t.dim() != 3:
        raise ValueError(f"{name} must be [X, Y, Z], got {tuple(t.shape)}")
    if t.dtype != dtype and not (dtype == torch.uint8 and t.dtype == torch.bool):
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    _reso3(list(t.shape), name + ".shape")
    return t.detach().contiguous()


def _refuse_half(grid, who):
    """``TypeError`` for a ``grid_half.HalfGrid`` where the fp32 SH table of a grid is read or written, and
    ``NotImplementedError`` for a ``grid_background.BackgroundGrid`` where only a foreground is handled."""
    if getattr(grid, "is_half", False):
        raise TypeError(f"{who} reads or writes the fp32 SH table of a SparseGrid and a HalfGrid has none: pass grid.to_float()")
    if getattr(grid, "is_palette", False):
        raise TypeError(f"{who} reads or writes the fp32 SH table of a SparseGrid and a PaletteGrid has none: pass grid.to_float()")
    if getattr(grid, "use_background", False):
        raise NotImplementedError(f"{who} is built for the foreground only (training, resampling and pruning a background are "
                                  "not): pass grid.foreground(), the SparseGrid on the same tensors")


def _as_u8(mask):
    """A bool mask as the uint8 bytes the kernels read (the same memory)."""
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


def _morton(n):
    """Morton code of every node of an n^3 cube (x in the highest bit of each triple), int64 ``[n, n, n]``."""
    a = np.arange(n, dtype=np.int64)
    spread = np.zeros(n, dtype=np.int64)
    for b in range(max(1, int(n).bit_length())):
        spread |= ((a >> b) & 1) << (3 * b)
    return (spread[:, None, None] << 2) + (spread[None, :, None] << 1) + spread[None, None, :]


class SparseGrid:
    """svox2.SparseGrid, forward side. ``links`` int32 ``[X, Y, Z]`` (``>= 0``: row of the data, any negative value: empty -
    values ``< -1`` are never read as skip distances), ``density_data`` ``[capacity, 1]``, ``sh_data``
    ``[capacity, 3 * basis_dim]``, all on the GPU. Any write to ``links`` - assigning it, or writing into it in place
    (``grid.links[mask] = -1``, also through an alias or a view) - drops the skip data of :meth:`accelerate` before the next
    call and has the new links checked against ``capacity`` again; so does assigning ``density_data`` or ``sh_data``.

    The tensors are borrowed by the C library (include/nerf_mi355x.h); this object keeps them alive."""

    def __init__(self, reso: Union[int, List[int], Tuple[int, int, int]] = 128, radius: Union[float, List[float]] = 1.0,
                 center: Union[float, List[float]] = [0.0, 0.0, 0.0], basis_type: int = BASIS_TYPE_SH, basis_dim: int = 9,
                 basis_reso: int = 16, use_z_order: bool = False, use_sphere_bound: bool = False, mlp_posenc_size: int = 0,
                 mlp_width: int = 16, background_nlayers: int = 0, background_reso: int = 256,
                 device: Union[torch.device, str] = "cuda"):
        self._init_common(reso, radius, center, basis_type, basis_dim, background_nlayers, device)
        reso = self._reso
        n3 = reso[0] * reso[1] * reso[2]
        dev = self.ctx.device
        cube_pow2 = reso[0] == reso[1] == reso[2] and reso[0] & (reso[0] - 1) == 0
        if use_z_order and not cube_pow2:
            import warnings
            warnings.warn(f"use_z_order needs a cubic grid with a power-of-two side, got {reso}: rows stay in C order")
            use_z_order = False
        # the row every node would get in a dense grid: its C-order index, or its Morton code
        order = (torch.from_numpy(_morton(reso[0])).to(dev) if use_z_order else torch.arange(n3, device=dev).view(reso)).flatten()
        if use_sphere_bound:
            # node i of an axis has the normalised coordinate 2 i / reso - 1; a node is kept when that point lies within
            # 1 + sqrt(3) / max(reso) of the origin (svox2's bound). Kept nodes are numbered by the rank of their dense row
            # among the kept ones, so that C order / Morton order survives the compaction.
            u = [2.0 * torch.arange(r, dtype=torch.float32, device=dev) / r - 1.0 for r in reso]
            dist = (u[0][:, None, None] ** 2 + u[1][None, :, None] ** 2 + u[2][None, None, :] ** 2).sqrt()
            inside = (dist <= 1.0 + 3.0 ** 0.5 / max(reso)).flatten()
            self.capacity = int(inside.sum())
            kept_nodes = inside.nonzero().flatten()
            by_row = torch.argsort(order[kept_nodes])
            rank = torch.empty_like(by_row)
            rank[by_row] = torch.arange(self.capacity, device=dev)
            init_links = torch.full((n3,), -1, dtype=torch.int32, device=dev)
            init_links[kept_nodes] = rank.to(torch.int32)
        else:
            self.capacity = n3
            init_links = order.to(torch.int32)
        self._density = torch.zeros((self.capacity, 1), dtype=torch.float32, device=dev)
        self._sh = torch.zeros((self.capacity, self.basis_dim * 3), dtype=torch.float32, device=dev)
        self._links = init_links.view(reso).contiguous()
        if use_sphere_bound:
            self.accelerate()

    def _init_common(self, reso, radius, center, basis_type, basis_dim, background_nlayers, device):
        self._handle_ptr = None
        self._handle_key = None
        if basis_type != BASIS_TYPE_SH:
            raise NotImplementedError(f"basis_type {basis_type}: only spherical harmonics (BASIS_TYPE_SH) are built, "
                                      "not the learned 3D texture or the MLP basis")
        if basis_dim not in (1, 4, 9):
            raise ValueError(f"basis_dim {basis_dim}: spherical harmonics of 1, 4 or 9 coefficients are built")
        if background_nlayers:
            raise NotImplementedError("background MSI layers are not built into SparseGrid: grid_background.BackgroundGrid has them")
        if torch.device(device).type != "cuda":
            raise RuntimeError(f"device {device} is not a GPU: SparseGrid has no CPU fallback")
        self.ctx = get_context(device)
        self.basis_type, self.basis_dim = basis_type, int(basis_dim)
        self.background_nlayers = 0
        reso = [int(reso)] * 3 if isinstance(reso, (int, np.integer)) else [int(r) for r in reso]
        if len(reso) != 3:
            raise ValueError("reso must be an integer or indexable object of 3 ints")
        self._reso = reso
        self.radius = _three(radius, "radius")      # fp32, CPU, as in svox2
        self.center = _three(center, "center")
        # grid = world * scale + shift with scale = reso * (0.5 / radius), shift = reso * (0.5 * (1 - center / radius)) - 0.5:
        # the fp32 values nerf_grid_create computes (include/nerf_mi355x.h)
        self._unit_scale = 0.5 / self.radius
        self._unit_shift = 0.5 * (1.0 - self.center / self.radius)
        self.opt = RenderOptions()

    @classmethod
    def from_tensors(cls, links, density_data, sh_data, radius, center, basis_dim=None):
        """A grid around existing device tensors (borrowed, no dense allocation): ``links`` int32 ``[X, Y, Z]``,
        ``density_data`` ``[capacity, 1]``, ``sh_data`` ``[capacity, 3 * basis_dim]``."""
        g = cls.__new__(cls)
        links = torch.as_tensor(links)
        if links.dim() != 3:
            raise ValueError(f"links must be [X, Y, Z], got shape {tuple(links.shape)}")
        if not links.is_cuda:
            raise RuntimeError("links is on the CPU: SparseGrid has no CPU fallback (pass device tensors)")
        sh_data = torch.as_tensor(sh_data)
        if sh_data.dim() != 2 or sh_data.shape[1] % 3:
            raise ValueError(f"sh_data must be [capacity, 3 * basis_dim], got shape {tuple(sh_data.shape)}")
        bd = sh_data.shape[1] // 3 if basis_dim is None else basis_dim
        g._init_common(list(links.shape), radius, center, BASIS_TYPE_SH, bd, 0, links.device)
        g.capacity = int(sh_data.shape[0])
        g._links, g._density, g._sh = links, torch.as_tensor(density_data), sh_data
        g._handle()      # validates
        return g

    def _like(self, links, density_data, sh_data, accelerate):
        """A new grid around three fresh tensors, with this grid's radius, center, basis and a copy of its ``opt``."""
        g = SparseGrid.__new__(SparseGrid)
        g._init_common(list(links.shape), self.radius, self.center, BASIS_TYPE_SH, self.basis_dim, 0, self.ctx.device)
        g.capacity = int(density_data.shape[0])
        g._links, g._density, g._sh = links, density_data, sh_data
        g.opt = replace(self.opt)
        if accelerate:
            g.accelerate()
        return g

    # ---- the borrowed tensors -------------------------------------------------------------------------------
    def _drop_handle(self):
        if getattr(self, "_handle_ptr", None) is not None:
            try:
                self.ctx.lib.nerf_grid_destroy(self._handle_ptr)
            except Exception:      # (interpreter shutdown)
                pass
        self._handle_ptr = None
        self._handle_key = None

    __del__ = _drop_handle

    @property
    def links(self):
        return self._links

    @links.setter
    def links(self, t):
        self._drop_handle()      # and with it the skip data
        self._links = t

    @property
    def density_data(self):
        return self._density

    @density_data.setter
    def density_data(self, t):
        self._drop_handle()
        self._density = t
        self.capacity = int(t.shape[0])

    @property
    def sh_data(self):
        return self._sh

    @sh_data.setter
    def sh_data(self, t):
        self._drop_handle()
        self._sh = t

    def _key(self):
        """What a handle (and its skip data) was made from: the three tensors' storage and shape, and the version counter of
        ``links``, which torch advances on every in-place write - through this object, an alias or a view alike."""
        tensors = (self._links, self._density, self._sh)
        if not all(torch.is_tensor(t) for t in tensors):
            return None
        return tuple((t.data_ptr(), tuple(t.shape)) for t in tensors) + (self._links._version,)

    def _handle(self):
        key = self._key()
        if self._handle_ptr is not None and key == self._handle_key:
            return self._handle_ptr
        self._drop_handle()
        L, D, S = self._links, self._density, self._sh
        for name, t, dt in (("links", L, torch.int32), ("density_data", D, torch.float32), ("sh_data", S, torch.float32)):
            if not torch.is_tensor(t):
                raise TypeError(f"{name} must be a tensor")
            if not t.is_cuda:
                raise RuntimeError(f"{name} is on the CPU: SparseGrid has no CPU fallback")
            if t.device != self.ctx.device:
                raise RuntimeError(f"{name} is on {t.device}, the grid on {self.ctx.device}")
            if t.dtype != dt:
                raise TypeError(f"{name} must be {dt}, got {t.dtype}")
            if not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
            if t.requires_grad:
                raise NotImplementedError("gradients through a SparseGrid (training the grid) are not built")
        cap = int(D.shape[0])
        if L.dim() != 3 or D.dim() != 2 or D.shape[1] != 1 or S.dim() != 2 or tuple(S.shape) != (cap, 3 * self.basis_dim):
            raise ValueError(f"mismatched shapes: links {tuple(L.shape)} [X, Y, Z], density_data {tuple(D.shape)} [capacity, 1], "
                             f"sh_data {tuple(S.shape)} [capacity, {3 * self.basis_dim}]")
        d = SparseGridDesc()
        d.reso[:] = list(L.shape)
        d.basis_dim = self.basis_dim
        d.radius[:] = self.radius.tolist()
        d.center[:] = self.center.tolist()
        d.capacity = cap
        d.links, d.density_data, d.sh_data = L.data_ptr(), D.data_ptr(), S.data_ptr()
        d.stream = self.ctx.stream().value
        h = C.c_void_p()
        check(self.ctx.lib.nerf_grid_create(self.ctx.handle, C.byref(d), C.byref(h)))
        self.capacity = cap
        self._handle_ptr, self._handle_key = h, key
        return h

    # ---- svox2's surface --------------------------------------------------------------------------------
    @property
    def data_dim(self):
        return self._sh.size(1) + 1

    @property
    def use_background(self):
        return False

    @property
    def shape(self):
        return list(self._links.shape) + [self.data_dim]

    @property
    def accelerated(self):
        """Whether skip data of :meth:`accelerate` is current."""
        return (self._handle_ptr is not None and self._key() == self._handle_key
                and bool(self.ctx.lib.nerf_grid_has_skip(self._handle_ptr)))

    def _affine(self, device):
        """``(scale, shift)`` of ``grid = world * scale + shift`` as fp32 tensors on ``device``."""
        n = torch.tensor([float(r) for r in self._links.shape], dtype=torch.float32)
        return (n * self._unit_scale).to(device), (n * self._unit_shift - 0.5).to(device)

    def world2grid(self, points):
        """World coordinates to grid coordinates: node ``i`` of an axis is at ``i``, the box is ``[-0.5, reso - 0.5]``."""
        scale, shift = self._affine(points.device)
        return points * scale + shift

    def grid2world(self, points):
        """The inverse of :meth:`world2grid`: node ``i`` sits at ``center - radius + (i + 0.5) * 2 radius / reso``."""
        scale, shift = self._affine(points.device)
        return (points - shift) / scale

    def _rays_arg(self, t, name, n=None):
        if not torch.is_tensor(t):
            raise TypeError(f"{name} must be a tensor")
        if not t.is_cuda:
            raise RuntimeError(f"{name} is on the CPU: SparseGrid has no CPU fallback")
        if t.requires_grad:
            raise NotImplementedError("gradients through a SparseGrid are not built")
        if t.dim() != 2 or t.shape[1] != 3 or (n is not None and t.shape[0] != n):
            raise ValueError(f"{name} must be [N, 3], got {tuple(t.shape)}")
        return t.detach().to(device=self.ctx.device, dtype=torch.float32).contiguous()

    def _render(self, cam, rays, randomize, return_log_transmit, counters):
        opt = self.opt._to_c(randomize)
        h = self._handle()
        a = GridRenderArgs()
        if cam is not None:
            c = cam._to_c()
            n = cam.width * cam.height
        else:
            o = self._rays_arg(rays.origins, "rays.origins")
            d = self._rays_arg(rays.dirs, "rays.dirs", o.shape[0])
            n = o.shape[0]
            a.origins, a.dirs, a.n_rays = o.data_ptr(), d.data_ptr(), n
        rgb = torch.empty((n, 3), device=self.ctx.device, dtype=torch.float32)
        logt = torch.empty((n,), device=self.ctx.device, dtype=torch.float32) if return_log_transmit else None
        a.rgb = rgb.data_ptr()
        a.log_transmit = 0 if logt is None else logt.data_ptr()
        a.counters = 0 if counters is None else counters.data_ptr()
        a.use_skip = 1
        a.stream = self.ctx.stream().value
        if cam is not None:
            check(self.ctx.lib.nerf_grid_render_image(h, C.byref(c), C.byref(opt), C.byref(a)))
        else:
            check(self.ctx.lib.nerf_grid_render_rays(h, C.byref(opt), C.byref(a)))
        return (rgb, logt) if return_log_transmit else rgb

    def _depth(self, cam, rays, mode, sigma_thresh=0.0, return_log_transmit=False, randomize=False):
        """One call of nerf_grid_depth_rays / nerf_grid_depth_image: ``depth [n]`` (and ``log_transmit [n]``)."""
        opt = self.opt._to_c(randomize)
        h = self._handle()
        a = GridDepthArgs()
        a.mode, a.sigma_thresh = mode, sigma_thresh
        if cam is not None:
            c = cam._to_c()
            n = cam.width * cam.height
        else:
            o = self._rays_arg(rays.origins, "rays.origins")
            d = self._rays_arg(rays.dirs, "rays.dirs", o.shape[0])
            n = o.shape[0]
            a.origins, a.dirs, a.n_rays = o.data_ptr(), d.data_ptr(), n
        depth = torch.empty((n,), device=self.ctx.device, dtype=torch.float32)
        logt = torch.empty((n,), device=self.ctx.device, dtype=torch.float32) if return_log_transmit else None
        a.depth = depth.data_ptr()
        a.log_transmit = 0 if logt is None else logt.data_ptr()
        a.use_skip = 1
        a.stream = self.ctx.stream().value
        if cam is not None:
            check(self.ctx.lib.nerf_grid_depth_image(h, C.byref(c), C.byref(opt), C.byref(a)))
        else:
            check(self.ctx.lib.nerf_grid_depth_rays(h, C.byref(opt), C.byref(a)))
        return (depth, logt) if return_log_transmit else depth

    @staticmethod
    def _depth_mode(sigma_thresh, return_log_transmit=False):
        if sigma_thresh is None:
            return _lib.NERF_GRID_DEPTH_EXPECTED, 0.0
        x = float(sigma_thresh)
        if not x >= 0.0:
            raise ValueError(f"sigma_thresh = {sigma_thresh!r} must be >= 0 and not NaN: the empty-space skip is only valid when "
                             "an empty cell (sigma == 0) can never be a hit")
        if return_log_transmit:
            raise ValueError("return_log_transmit belongs to the expected termination (sigma_thresh=None)")
        return _lib.NERF_GRID_DEPTH_THRESHOLD, x

    def volume_render(self, rays: Rays, use_kernel: bool = True, randomize: bool = False, return_raylen: bool = False,
                      return_log_transmit: bool = False):
        """``[N, 3]`` colours of ``rays`` (``dirs`` need not be unit) under ``self.opt``; with ``return_log_transmit`` also the
        log of the transmittance left at the end of every ray (exactly -1e3 where the ray stopped at ``stop_thresh``).
        With ``return_raylen`` nothing is rendered: ``[N]``, the length ``tmax - tmin`` of every ray inside the box in grid
        units (``near_clip`` applied; negative for a miss, NaN for a ray that is not finite), as svox2's PyTorch renderer."""
        if not use_kernel:
            raise NotImplementedError("use_kernel=False (the PyTorch renderer) does not exist here: HIP kernels only")
        if return_raylen:
            if return_log_transmit:
                raise ValueError("return_raylen marches nothing: there is no log_transmit to return")
            return self._depth(None, rays, _lib.NERF_GRID_DEPTH_RAYLEN, randomize=randomize)
        return self._render(None, rays, randomize, return_log_transmit, None)

    def volume_render_image(self, camera: Camera, use_kernel: bool = True, randomize: bool = False, batch_size: int = 5000,
                            return_raylen: bool = False):
        """``[H, W, 3]``: the rays of ``camera`` are made inside the render launch, a frame is one C call (``batch_size`` is
        accepted for the call surface). With ``return_raylen``: ``[H, W, 1]``, the ray lengths of :meth:`volume_render`."""
        if not use_kernel:
            raise NotImplementedError("use_kernel=False (the PyTorch renderer) does not exist here: HIP kernels only")
        if return_raylen:
            return self._depth(camera, None, _lib.NERF_GRID_DEPTH_RAYLEN, randomize=randomize).view(camera.height, camera.width, 1)
        return self._render(camera, None, randomize, False, None).view(camera.height, camera.width, 3)

    def volume_render_depth(self, rays: Rays, sigma_thresh: Optional[float] = None, return_log_transmit: bool = False):
        """``[N]`` depths of ``rays`` in world units along the ray (not z-depth), on the sample lattice of :meth:`volume_render`.
        ``sigma_thresh=None``: the expected termination ``sum_i weight_i t_i`` under ``self.opt`` - not divided by the
        accumulated opacity; with ``return_log_transmit`` also ``log_transmit [N]`` (the render's, bit for bit), so that
        ``depth / (1 - exp(log_transmit))`` normalises it. ``sigma_thresh=x`` (``x >= 0``): the distance of the first
        sample whose density strictly exceeds ``x``. 0 where nothing is hit."""
        mode, x = self._depth_mode(sigma_thresh, return_log_transmit)
        return self._depth(None, rays, mode, x, return_log_transmit)

    def volume_render_depth_image(self, camera: Camera, sigma_thresh: Optional[float] = None, batch_size: int = 5000):
        """``[H, W]``: :meth:`volume_render_depth` of the rays of ``camera``, made inside the launch; a frame is one C call
        (``batch_size`` is accepted for the call surface)."""
        mode, x = self._depth_mode(sigma_thresh)
        return self._depth(camera, None, mode, x).view(camera.height, camera.width)

    def count_samples(self, camera=None, rays=None):
        """``(visited, shaded)`` samples of a render, counted in an instrumented launch of its own (atomics; waits)."""
        counters = torch.zeros(2, device=self.ctx.device, dtype=torch.int64)
        self._render(camera, rays, False, False, counters)
        v, s = counters.cpu().tolist()
        return v, s

    def sample(self, points: torch.Tensor, use_kernel: bool = True, grid_coords: bool = False, want_colors: bool = True):
        """Trilinear sampling like ``grid_sample`` with border padding and ``align_corners=False``; empty nodes are zero.
        ``(density [N, 1], sh [N, 3 * basis_dim])`` (``sh`` empty without ``want_colors``). ``points`` is not modified."""
        if not use_kernel:
            raise NotImplementedError("use_kernel=False (the PyTorch sampler) does not exist here: HIP kernels only")
        p = self._rays_arg(points, "points")
        h = self._handle()
        n = p.shape[0]
        dens = torch.empty((n, 1), device=self.ctx.device, dtype=torch.float32)
        sh = torch.empty((n if want_colors else 0, 3 * self.basis_dim), device=self.ctx.device, dtype=torch.float32)
        a = GridSampleArgs()
        a.points, a.n, a.grid_coords, a.want_colors = p.data_ptr(), n, int(bool(grid_coords)), int(bool(want_colors))
        a.density, a.sh = dens.data_ptr(), sh.data_ptr() if want_colors else 0
        a.stream = self.ctx.stream().value
        check(self.ctx.lib.nerf_grid_sample(h, C.byref(a)))
        return dens, sh

    def forward(self, points: torch.Tensor, use_kernel: bool = True):
        return self.sample(points, use_kernel=use_kernel)

    __call__ = forward

    def to_half(self, lanes=None):
        """``grid_half.HalfGrid.from_grid(self)``: the inference twin of this grid with its colours in fp16 on the device."""
        from .grid_half import HalfGrid
        return HalfGrid.from_grid(self, lanes=lanes)

    def to_palette(self, bits=16, retain=0, sigma_thresh=None):
        """``grid_palette.PaletteGrid.from_grid(self, ...)``: the inference twin of this grid with one palette index per node
        and basis function in place of its colours."""
        from .grid_palette import PaletteGrid
        return PaletteGrid.from_grid(self, bits=bits, retain=retain, sigma_thresh=sigma_thresh)

    def accelerate(self):
        """Build the empty-space skip data on the device from the CURRENT links (a separate array; ``links`` is not written)."""
        check(self.ctx.lib.nerf_grid_accelerate(self._handle(), self.ctx.stream()))

    def save(self, path: str, compress: bool = False):
        """svox2's ``.npz``: ``radius``, ``center``, ``links``, ``density_data``, ``sh_data`` (fp16), ``basis_type``. Every
        negative link is written as -1: this object's skip data lives outside ``links``, and values ``< -1`` that arrived
        from elsewhere are not the reference's skip encoding."""
        links = self._links.detach().cpu().numpy()
        data = {
            "radius": self.radius.numpy(),
            "center": self.center.numpy(),
            "links": np.where(links < 0, np.int32(-1), links).astype(np.int32),
            "density_data": self._density.detach().cpu().numpy(),
            "sh_data": self._sh.detach().cpu().numpy().astype(np.float16),
            "basis_type": self.basis_type,
        }
        (np.savez_compressed if compress else np.savez)(path, **data)

    @staticmethod
    def read_npz(path):
        """The arrays of svox2's ``.npz`` (also the old layout with one ``data`` array, density first) as numpy, on the host:
        ``links`` int32, ``density_data`` / ``sh_data`` fp32 (stored fp16 is widened), ``radius``, ``center``. Refuses what is
        not built (background layers, learned bases)."""
        z = np.load(path)
        if "background_data" in z.files:
            raise NotImplementedError("background MSI layers are not built into SparseGrid: grid_background.load_grid / "
                                      "BackgroundGrid.load open this file")
        basis_type = int(z["basis_type"].item()) if "basis_type" in z.files else BASIS_TYPE_SH
        if basis_type != BASIS_TYPE_SH or "basis_data" in z.files:
            raise NotImplementedError("only spherical harmonics (BASIS_TYPE_SH) are built, not learned bases")
        if "data" in z.files:
            sh_data, density_data = z["data"][..., 1:], z["data"][..., :1]
        else:
            sh_data, density_data = z["sh_data"], z["density_data"]
        host = lambda a, dt: np.ascontiguousarray(np.asarray(a).astype(dt))      # noqa: E731
        return {"links": host(z["links"], np.int32), "density_data": host(density_data, np.float32),
                "sh_data": host(sh_data, np.float32),
                "radius": z["radius"].tolist() if "radius" in z.files else [1.0, 1.0, 1.0],
                "center": z["center"].tolist() if "center" in z.files else [0.0, 0.0, 0.0]}

    @classmethod
    def load(cls, path: str, device: Union[torch.device, str] = "cuda"):
        """A grid from svox2's ``.npz`` (:meth:`read_npz`). Links ``< -1`` in the file are read as empty; call
        :meth:`accelerate` for skip data."""
        a = cls.read_npz(path)
        if torch.device(device).type != "cuda":
            raise RuntimeError(f"device {device} is not a GPU: SparseGrid has no CPU fallback")
        dev = get_context(device).device
        return cls.from_tensors(*(torch.from_numpy(a[k]).to(dev) for k in ("links", "density_data", "sh_data")),
                                a["radius"], a["center"])

    # ---- what svox2 has and this module does not --------------------------------------------------------
    def _not_built(name, what):      # noqa: N805
        def f(self, *a, **k):
            raise NotImplementedError(f"SparseGrid.{name}: {what} is not built")
        f.__name__ = name
        return f

    volume_render_fused = _not_built("volume_render_fused", "grid training (fused backward)")
    resample = _not_built("resample", "resampling / upsampling")
    sparsify_background = _not_built("sparsify_background", "background MSI layers")
    tv = _not_built("tv", "grid training (total-variation loss)")
    tv_color = _not_built("tv_color", "grid training (total-variation loss)")
    inplace_tv_grad = _not_built("inplace_tv_grad", "grid training (total-variation loss)")
    optim_density_step = _not_built("optim_density_step", "grid training (optimiser)")
    optim_sh_step = _not_built("optim_sh_step", "grid training (optimiser)")
    # (the conversion exists under a name of its own, like training: octree.N3Tree.from_grid(grid); this svox2-named method
    # keeps raising, as the other svox2-named methods here do)
    to_svox1 = _not_built("to_svox1", "the svox2-named conversion (octree.N3Tree.from_grid(grid) builds the octree)")
    del _not_built

    # ---- baking -----------------------------------------------------------------------------------------
    @classmethod
    def from_nerf(cls, network, c1, c2, reso, *, basis_dim=9, occupancy=None, threshold=0.0, dilate=1, n_dirs=64,
                  chunk=32768, white_bkgd=True):
        """Bake ``network`` (this package's ``NeRF``; use the fine model) into a grid over the box ``[c1, c2]``.

        Geometry: ``radius = (c2 - c1) / 2``, ``center = (c1 + c2) / 2``; node ``i`` sits at the voxel centre
        ``grid2world(i)``. Sigma comes from ``density_grid`` on the lattice whose end points are the first and last voxel
        centres, ``lo = c1 + (c2 - c1) / (2 reso)``, ``hi = c2 - (c2 - c1) / (2 reso)``; its ``np.linspace`` fp32
        coordinates are authoritative for the bake (the colour evaluations use the same points). They differ from the fp32
        ``grid2world(i)`` by an ulp at most, immaterial for a bake.

        Sparsity: an ``OccupancyGrid`` on that same lattice (built here from ``threshold`` / ``dilate``, or passed in -
        ``ValueError`` if it is on another lattice); a node is kept iff one of the up to 8 cells touching it is occupied.
        ``links`` = running index over the kept nodes in C order, else -1. ``density_data`` = ``density_grid``'s value at
        the node, bit for bit.

        Colour: at every kept node the network is evaluated for the ``n_dirs`` directions of
        ``fibonacci_directions(n_dirs)`` through ``run_network`` (in chunks of ``chunk`` nodes), and the samples are
        projected by the kernel ``nerf_grid_project_sh``: ``c = P (sigmoid(rgb_raw) - 0.5)`` per channel with
        ``P = pinv(Y)`` computed in fp64 and rounded to fp32 (``sh_projection_matrix``), the counterpart of the grid's
        colour model ``max(0, c . Y + 0.5)``. With the default ``n_dirs = 64`` the basis matrix ``Y`` of degree 2 has
        condition number 1.014 (1.055 at 32 directions, 1.005 at 128): ``P`` is a plain quadrature up to a per cent and
        noise in the samples is averaged down by ``|P row|_2 = sqrt(4 pi / n_dirs) = 0.44``, not amplified; 64 is the
        point past which the conditioning no longer improves noticeably while the bake's cost keeps growing linearly.
        The trunk is evaluated again for every direction; that is accepted for a one-off bake (about
        ``kept nodes * n_dirs / 3.6e8`` seconds). A model without view directions has one colour per node:
        ``basis_dim`` is forced to 1 and the node is evaluated once.

        ``white_bkgd`` of the NeRF render maps to ``opt.background_brightness`` 1.0 / 0.0. The grid renders everything
        inside the box, whereas ``render()`` only looks between ``near`` and ``far``."""
        if not isinstance(network, NeRF):
            raise TypeError("SparseGrid.from_nerf needs this package's NeRF")
        c1, c2, reso = _axes(c1, c2, reso)
        if any(r < 2 for r in reso) or any(b <= a for a, b in zip(c1, c2)):
            raise ValueError("from_nerf: reso >= 2 per axis and c2 > c1 are required")
        lo = [a + (b - a) / (2 * r) for a, b, r in zip(c1, c2, reso)]
        hi = [b - (b - a) / (2 * r) for a, b, r in zip(c1, c2, reso)]
        if not network.use_viewdirs:
            basis_dim, n_dirs = 1, 1
        if basis_dim not in (1, 4, 9):
            raise ValueError(f"basis_dim {basis_dim}: spherical harmonics of 1, 4 or 9 coefficients are built")
        ctx = network.ctx
        dev = ctx.device
        with torch.no_grad():
            sigma = density_grid(network, lo, hi, reso)
            if occupancy is None:      # from the lattice just evaluated (OccupancyGrid.build would evaluate it again)
                occupancy = OccupancyGrid(ctx, lo, hi, reso, [sigma], None, threshold, dilate, "empty")
            elif (list(occupancy.c1), list(occupancy.c2), list(occupancy.reso)) != (lo, hi, reso) or occupancy.ctx is not ctx:
                raise ValueError(f"from_nerf: the occupancy grid must be on the bake's lattice: c1 = {lo}, c2 = {hi}, "
                                 f"reso = {reso} (got {occupancy.c1}, {occupancy.c2}, {occupancy.reso})")
            cells = occupancy.cells()
            pad = torch.zeros([r + 1 for r in reso], dtype=torch.bool, device=dev)
            pad[1:-1, 1:-1, 1:-1] = cells
            kept = torch.zeros(reso, dtype=torch.bool, device=dev)
            for a in (0, 1):
                for b in (0, 1):
                    for c in (0, 1):
                        kept |= pad[a:a + reso[0], b:b + reso[1], c:c + reso[2]]
            flat = kept.flatten()
            links = torch.where(flat, torch.cumsum(flat.to(torch.int32), 0, dtype=torch.int32) - 1,
                                torch.full_like(flat, -1, dtype=torch.int32)).view(reso).contiguous()
            idx = flat.nonzero().flatten()
            cap = int(idx.numel())
            density = sigma.flatten()[idx].reshape(cap, 1).contiguous()
            sh = torch.zeros((cap, 3 * basis_dim), dtype=torch.float32, device=dev)
            if cap:
                axes = [torch.from_numpy(np.linspace(l, h, n, dtype=np.float32)).to(dev) for l, h, n in zip(lo, hi, reso)]
                iz = idx % reso[2]
                iy = (idx // reso[2]) % reso[1]
                ix = idx // (reso[1] * reso[2])
                pts = torch.stack([axes[0][ix], axes[1][iy], axes[2][iz]], -1)
                P, _, dirs = sh_projection_matrix(basis_dim, n_dirs)
                P32 = torch.from_numpy(P.astype(np.float32)).to(dev).contiguous()
                cls._bake_colours(network, pts, dirs, P32, sh, basis_dim, chunk)
        g = cls.from_tensors(links, density, sh, [(b - a) / 2 for a, b in zip(c1, c2)], [(a + b) / 2 for a, b in zip(c1, c2)],
                            basis_dim=basis_dim)
        g.opt.background_brightness = 1.0 if white_bkgd else 0.0
        return g

    @staticmethod
    def bake_raw(network, pts, dirs):
        """What the bake projects: ``raw [M, n_dirs, 4]`` of ``network`` at ``pts [M, 3]`` for the unit directions
        ``dirs [n_dirs, 3]`` (``[M, 1, 4]`` for a model without view directions), through ``run_network``."""
        ctx = network.ctx
        m = pts.shape[0]
        embed = get_embedder((network.input_ch - 3) // 6, 0 if network.input_ch > 3 else -1)[0]
        if not network.use_viewdirs:
            return run_network(pts.reshape(m, 1, 3), None, network, embed, None)[..., :4].contiguous()
        embeddirs = get_embedder((network.input_ch_views - 3) // 6, 0 if network.input_ch_views > 3 else -1)[0]
        vd = torch.as_tensor(np.asarray(dirs, dtype=np.float32), device=ctx.device)
        n = vd.shape[0]
        raw = run_network(pts[None].expand(n, m, 3).contiguous(), vd, network, embed, embeddirs)      # [n_dirs, M, 4]
        return raw.permute(1, 0, 2).contiguous()

    @classmethod
    def _bake_colours(cls, network, pts, dirs, P32, sh, basis_dim, chunk):
        ctx = network.ctx
        n_dirs = P32.shape[1]
        for r0 in range(0, pts.shape[0], chunk):
            raw = cls.bake_raw(network, pts[r0:r0 + chunk], dirs)
            a = GridProjectArgs()
            a.raw, a.m, a.n_dirs, a.basis_dim = raw.data_ptr(), raw.shape[0], n_dirs, basis_dim
            a.P, a.sh_out, a.row0 = P32.data_ptr(), sh.data_ptr(), r0
            a.stream = ctx.stream().value
            check(ctx.lib.nerf_grid_project_sh(ctx.handle, C.byref(a)))
