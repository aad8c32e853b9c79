"""Coloured surface meshes of a sparse voxel grid (Plenoxels), extracted on the GPU.

``extract_mesh(grid, isovalue)`` is marching cubes on the grid's own lattice - the kernels of ``marching_cubes_volume`` reading
``links`` and ``density_data`` in place of a dense volume, so no volume is materialised and no resampling error enters - with a
normal and a colour at every vertex from a second kernel, ``mesh_attributes``, which also serves any other points (a point
cloud). Semantics: include/nerf_mi355x.h, "Sparse voxel grid: surface meshes"; kernels: csrc/mesh_kernels.hip and
csrc/grid_mesh_kernels.hip. As everywhere in this package there is no CPU or PyTorch fallback.

    mesh = extract_mesh(grid, 10.0)                        # SparseGrid, HalfGrid, PaletteGrid or BackgroundGrid (foreground only)
    mesh.vertices [V, 3] fp32    mesh.triangles [T, 3] int64    mesh.normals [V, 3] fp32    mesh.colors [V, 3] fp32 in [0, 1]
    mesh.save_obj("lego.obj");  mesh.save_ply("lego.ply")

The geometry equals ``marching_cubes_volume(V, isovalue)`` for the volume ``V`` = the node densities with 0 at empty and
masked-out nodes, bit for bit and in order; ``isovalue`` must be > 0 so that an empty node is outside.

Only the object, without floaters: the connected-component labels of ``grid_components`` make the mask, in one call and with
no new code::

    labels, vol = label_components(grid, threshold=iso)
    mask = labels == (vol.argmax() + 1)
    mesh = extract_mesh(grid, iso, mask=mask)

A masked-out node has the value 0. With the labels cut at the isovalue itself, as above, a component's boundary is where the
surface runs anyway and the mesh is closed. A mask cut at another threshold, or any mask that runs through the inside region,
leaves cut faces along its boundary: the surface is closed there by flat faces that are not part of the object.
"""
import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib, mesh as _mesh
from ._lib import GridMcArgs, GridMeshAttributesArgs, check
from .grid import Rays, SparseGrid, _as_u8, _volume_arg
from .host import to8b

__all__ = ["GridMesh", "extract_mesh", "mesh_attributes", "render_colors"]


@dataclass
class GridMesh:
    """What :func:`extract_mesh` returns: device tensors. ``normals`` / ``colors`` are ``None`` when they were not asked for."""
    vertices: torch.Tensor
    triangles: torch.Tensor
    normals: Optional[torch.Tensor] = None
    colors: Optional[torch.Tensor] = None

    def save_obj(self, path):
        """Wavefront OBJ, exactly what ``mesh.save_obj(vertices, triangles, path, vert_rgb=colors)`` writes (normals are not
        part of that format as gen_mesh writes it)."""
        _mesh.save_obj(self.vertices, self.triangles, path, self.colors)

    def save_ply(self, path):
        """Binary little-endian PLY: per vertex float ``x y z``, float ``nx ny nz`` when there are normals, uchar
        ``red green blue`` (``to8b`` of the colours) when there are colours; per face a ``uchar`` count and three ``int``
        ``vertex_indices``."""
        v = self.vertices.detach().cpu().numpy().astype("<f4")
        t = self.triangles.detach().cpu().numpy()
        if v.shape[0] >= 2 ** 31:
            raise ValueError("a PLY face holds int32 vertex indices")
        fields, props = [("xyz", "<f4", 3)], ["property float x", "property float y", "property float z"]
        if self.normals is not None:
            fields.append(("n", "<f4", 3))
            props += ["property float nx", "property float ny", "property float nz"]
        if self.colors is not None:
            fields.append(("rgb", "u1", 3))
            props += ["property uchar red", "property uchar green", "property uchar blue"]
        vert = np.zeros(v.shape[0], dtype=np.dtype(fields))
        vert["xyz"] = v
        if self.normals is not None:
            vert["n"] = self.normals.detach().cpu().numpy()
        if self.colors is not None:
            vert["rgb"] = to8b(self.colors.detach().cpu().numpy())
        face = np.zeros(t.shape[0], dtype=np.dtype([("count", "u1"), ("v", "<i4", 3)]))
        face["count"] = 3
        face["v"] = t
        header = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}"] + props
        header += [f"element face {t.shape[0]}", "property list uchar int vertex_indices", "end_header"]
        with open(path, "wb") as fh:
            fh.write(("\n".join(header) + "\n").encode("ascii"))
            fh.write(vert.tobytes())
            fh.write(face.tobytes())


def _check_grid(grid, who):
    if not isinstance(grid, SparseGrid):
        raise TypeError(f"{who} needs a SparseGrid, HalfGrid, PaletteGrid or BackgroundGrid")
    return grid._handle()      # CPU tensors, wrong dtypes and shapes are refused here


def _check_iso(isovalue):
    iso = float(np.float32(isovalue))
    if not (iso > 0.0 and np.isfinite(iso)):
        raise ValueError(f"isovalue = {isovalue!r} must be finite and > 0 (in fp32): an empty node has the value 0 and must be outside")
    return iso


def _check_mask(grid, mask):
    if mask is None:
        return None
    m = _volume_arg(mask, "mask", torch.uint8, grid.ctx)
    if tuple(m.shape) != tuple(grid.links.shape):
        raise ValueError(f"mask must have the shape of links {tuple(grid.links.shape)}, got {tuple(m.shape)}")
    return _as_u8(m)


def _check_colors(colors, view=None, render=False):
    """``(mode, view)``: a NERF_GRID_MESH_COLOR_* mode (``"render"`` stays a string) and the fp32 unit direction."""
    if view is not None:
        if colors != "sh":
            raise ValueError("view gives the direction of colors='sh'; it has no meaning with another mode")
        colors = view
    if colors is None:
        return _lib.NERF_GRID_MESH_COLOR_NONE, None
    if isinstance(colors, str):
        if colors == "dc":
            return _lib.NERF_GRID_MESH_COLOR_DC, None
        if colors == "sh":
            return _lib.NERF_GRID_MESH_COLOR_SH, None
        if colors == "render" and render:
            return "render", None
        raise ValueError(f"colors = {colors!r}: expected 'sh', 'dc'" + (", 'render'" if render else "") +
                         ", a direction (dx, dy, dz) or None")
    try:
        d = np.asarray([float(x) for x in colors], dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"colors = {colors!r}: expected 'sh', 'dc'" + (", 'render'" if render else "") +
                         ", a direction (dx, dy, dz) or None") from None
    n = np.sqrt(np.sum(d * d)) if d.shape == (3,) else 0.0
    if not (np.isfinite(n) and n > 0.0):
        raise ValueError(f"colors = {colors!r}: a direction needs three finite values, not all zero")
    return _lib.NERF_GRID_MESH_COLOR_VIEW, (d / n).astype(np.float32)


def _points_arg(grid, points):
    if not torch.is_tensor(points):
        raise TypeError("points_index must be a tensor")
    if not points.is_cuda:
        raise RuntimeError("points_index is on the CPU: mesh_attributes has no CPU fallback")
    if points.device != grid.ctx.device:
        raise RuntimeError(f"points_index is on {points.device}, the grid on {grid.ctx.device}")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points_index must be [N, 3], got {tuple(points.shape)}")
    return points.detach().to(dtype=torch.float32).contiguous()


def _attributes(grid, h, p, mask, mode, view, want_normals):
    ctx = grid.ctx
    n = p.shape[0]
    normals = torch.empty((n, 3), device=ctx.device, dtype=torch.float32) if want_normals else None
    colors = torch.empty((n, 3), device=ctx.device, dtype=torch.float32) if mode != _lib.NERF_GRID_MESH_COLOR_NONE else None
    if n and (normals is not None or colors is not None):
        a = GridMeshAttributesArgs()
        a.points, a.n = p.data_ptr(), n
        a.mask = 0 if mask is None else mask.data_ptr()
        a.color_mode = mode
        if view is not None:
            a.view[:] = view.tolist()
        a.normals = 0 if normals is None else normals.data_ptr()
        a.colors = 0 if colors is None else colors.data_ptr()
        a.stream = ctx.stream().value
        check(ctx.lib.nerf_grid_mesh_attributes(h, C.byref(a)))
    return normals, colors


def mesh_attributes(grid, points_index, *, mask=None, colors="sh", view=None):
    """``(normals [N, 3], colors [N, 3] | None)`` at ``points_index`` ``[N, 3]``, device points in index (grid) coordinates -
    mesh vertices or any others. The normal is ``-grad sigma / |grad sigma|`` in world units (so anisotropic boxes come out
    right), the gradient interpolated trilinearly from central differences at the 8 nodes of the point's cell, with empty
    and masked-out (``mask``: uint8 / bool ``[X, Y, Z]``) nodes at 0; ``(0, 0, 0)`` where the gradient vanishes. ``colors``:
    ``"sh"`` evaluates the point's SH row - the one ``grid.sample(points, grid_coords=True)`` returns, from this grid
    class's own table - along ``-normal``, the ray that meets the surface head-on (or along ``view=(dx, dy, dz)``, one fixed
    direction; a tuple as ``colors`` means the same); ``"dc"`` is the constant term alone; ``None`` skips the colours."""
    h = _check_grid(grid, "mesh_attributes")
    mode, d = _check_colors(colors, view)
    m = _check_mask(grid, mask)
    p = _points_arg(grid, points_index)
    return _attributes(grid, h, p, m, mode, d, True)


def render_colors(grid, points_index, normals, dc, render_offset=1.5):
    """The ``"render"`` colours, a plain composition of existing calls: every point is looked at head-on by one ray of
    ``grid.volume_render`` that starts ``render_offset`` voxels outside the surface. With ``s`` the grid's fp32
    world-to-grid scale, ``n_index = (normals / s) / |normals / s|`` is the unit normal in index space and

        rgb = grid.volume_render(Rays(grid.grid2world(points_index + render_offset * n_index), -normals)).clamp(0, 1)

    Points whose normal is ``(0, 0, 0)`` take their row of ``dc``."""
    scale, _ = grid._affine(points_index.device)
    zero = (normals == 0).all(dim=1, keepdim=True)
    n_index = normals / scale
    n_index = torch.where(zero, torch.zeros_like(n_index), n_index / n_index.norm(dim=1, keepdim=True))
    origins = grid.grid2world(points_index + render_offset * n_index)
    rgb = grid.volume_render(Rays(origins, -normals)).clamp(0.0, 1.0)
    return torch.where(zero, dc, rgb)


def _mc_call(grid, h, iso, mask, verts=None, tris=None):
    n_v, n_t = C.c_int64(), C.c_int64()
    a = GridMcArgs()
    a.mask = 0 if mask is None else mask.data_ptr()
    a.iso = iso
    a.vertices = 0 if verts is None else verts.data_ptr()
    a.vertex_capacity = 0 if verts is None else verts.shape[0]
    a.triangles = 0 if tris is None else tris.data_ptr()
    a.triangle_capacity = 0 if tris is None else tris.shape[0]
    a.n_vertices, a.n_triangles = C.pointer(n_v), C.pointer(n_t)
    a.stream = grid.ctx.stream().value
    check(grid.ctx.lib.nerf_grid_marching_cubes(h, C.byref(a)))
    return n_v.value, n_t.value


def extract_mesh(grid, isovalue, *, mask=None, normals=True, colors="sh", world=True, render_offset=1.5):
    """The surface ``density == isovalue`` of ``grid`` as a :class:`GridMesh` of device tensors. Inside is
    ``density >= isovalue``; empty nodes and nodes where ``mask`` (uint8 / bool ``[X, Y, Z]``, e.g. one connected component:
    see the module text) is 0 count as density 0, so ``isovalue`` must be finite and > 0. Vertices and triangles are those of
    ``marching_cubes_volume`` on the densified volume, bit for bit and in its order: welded, deterministic, right-hand
    normals pointing out of the inside region.

    ``world=True`` returns ``grid.grid2world(v)`` of the index-coordinate vertices ``v`` that ``world=False`` returns.
    ``normals`` / ``colors`` as :func:`mesh_attributes` at the vertices (``colors`` also takes a direction ``(dx, dy, dz)``),
    and ``colors="render"`` looks at every vertex with the renderer itself: :func:`render_colors`."""
    h = _check_grid(grid, "extract_mesh")
    iso = _check_iso(isovalue)
    mode, d = _check_colors(colors, render=True)
    m = _check_mask(grid, mask)
    dev = grid.ctx.device
    n_v, n_t = _mc_call(grid, h, iso, m)
    verts = torch.empty((n_v, 3), device=dev, dtype=torch.float32)
    tris = torch.empty((n_t, 3), device=dev, dtype=torch.int64)
    if n_v and n_t:
        _mc_call(grid, h, iso, m, verts, tris)
    vert_normals = vert_colors = None
    if mode == "render":
        vert_normals, dc = _attributes(grid, h, verts, m, _lib.NERF_GRID_MESH_COLOR_DC, None, True)
        vert_colors = render_colors(grid, verts, vert_normals, dc, render_offset) if n_v else dc
        if not normals:
            vert_normals = None
    else:
        vert_normals, vert_colors = _attributes(grid, h, verts, m, mode, d, bool(normals))
    return GridMesh(grid.grid2world(verts) if world else verts, tris, vert_normals, vert_colors)
