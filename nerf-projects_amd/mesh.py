"""Mesh extraction from a NeRF's density field (plenoctree/nerf_sh/gen_mesh.py:88-158) on the GPU.

``marching_cubes(fn, c1, c2, reso, isosurface)`` is gen_mesh's function of the same name: sigma on a regular lattice
(``density_grid``, the fused encode+MLP kernel evaluating lattice nodes in place of a point buffer), marching cubes on
the device (``marching_cubes_volume``, in place of ``mcubes.marching_cubes``), and the reference's rescaling of the
vertices. ``save_obj`` writes the same text as gen_mesh's. Conventions (node order, vertex interpolation, winding,
ordering) are stated in include/nerf_mi355x.h, "Mesh extraction".
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import GridArgs, McArgs, check
from .host import NeRF, get_context

__all__ = ["density_grid", "marching_cubes_volume", "marching_cubes", "save_obj"]


def _axes(c1, c2, reso):
    """A scalar corner or resolution stands for all three axes (gen_mesh.py:167-175)."""
    def three(v, cast):
        vals = [cast(x) for x in np.atleast_1d(np.asarray(v)).tolist()]
        if len(vals) == 1:
            vals *= 3
        if len(vals) != 3:
            raise ValueError(f"expected a scalar or three values, got {v!r}")
        return vals
    return three(c1, float), three(c2, float), three(reso, int)


def density_grid(network, c1, c2, reso, chunk=None):
    """sigma = relu(raw[..., 3]) of ``network`` (this package's ``NeRF``, coarse or fine: gen_mesh's ``--coarse``) on the
    lattice ``meshgrid(*(np.linspace(lo, hi, n, dtype=np.float32) ...), indexing="ij")`` (gen_mesh.py:104-119), as a
    device tensor ``[X, Y, Z]``. One launch evaluates the whole lattice; ``chunk`` (gen_mesh's eval batch) does not change
    the result and is accepted for the call surface only. When the fp16-pair kernel's scale bound was loose the lattice is
    evaluated again in fp32 and a RuntimeWarning says so (the guard ``render()`` uses)."""
    if not isinstance(network, NeRF):
        raise TypeError("density_grid needs this package's NeRF")
    c1, c2, reso = _axes(c1, c2, reso)
    ctx = network.ctx
    sigma = torch.empty(tuple(reso), device=ctx.device, dtype=torch.float32)
    g = GridArgs()
    g.c1[:], g.c2[:], g.reso[:] = c1, c2, reso
    g.slot = network.slot
    g.sigma = sigma.data_ptr()
    g.stream = ctx.stream().value
    g.precision_guard = _lib.NERF_GUARD_FALLBACK
    check(ctx.lib.nerf_density_grid(ctx.handle, C.byref(g)))
    return sigma


def _mc_call(ctx, vol, iso, verts=None, tris=None):
    n_v, n_t = C.c_int64(), C.c_int64()
    a = McArgs()
    a.volume = vol.data_ptr()
    a.reso[:] = list(vol.shape)
    a.iso = float(iso)
    a.vertices = 0 if verts is None else verts.data_ptr()
    a.vertex_capacity = 0 if verts is None else verts.shape[0]
    a.triangles = 0 if tris is None else tris.data_ptr()
    a.triangle_capacity = 0 if tris is None else tris.shape[0]
    a.n_vertices, a.n_triangles = C.pointer(n_v), C.pointer(n_t)
    a.stream = ctx.stream().value
    check(ctx.lib.nerf_marching_cubes(ctx.handle, C.byref(a)))
    return n_v.value, n_t.value


def marching_cubes_volume(volume, isovalue):
    """``mcubes.marching_cubes(volume, isovalue)`` on the GPU: ``(vertices [V, 3] fp32, triangles [T, 3] int64)`` as device
    tensors, vertices in index coordinates. Inside is ``volume >= isovalue``; one vertex per crossing lattice edge; the
    triangles' right-hand normals point out of the inside region; the order is deterministic (include/nerf_mi355x.h)."""
    if not torch.is_tensor(volume) or not volume.is_cuda:
        ctx = get_context()
        volume = torch.as_tensor(np.asarray(volume, dtype=np.float32), device=ctx.device)
    else:
        ctx = get_context(volume.device)
    if volume.dim() != 3:
        raise ValueError(f"expected a volume [X, Y, Z], got shape {tuple(volume.shape)}")
    vol = volume.detach().to(dtype=torch.float32).contiguous()
    n_v, n_t = _mc_call(ctx, vol, isovalue)
    verts = torch.empty((n_v, 3), device=ctx.device, dtype=torch.float32)
    tris = torch.empty((n_t, 3), device=ctx.device, dtype=torch.int64)
    if n_v and n_t:
        _mc_call(ctx, vol, isovalue, verts, tris)
    return verts, tris


def marching_cubes(fn, c1, c2, reso, isosurface, chunk=720720):
    """gen_mesh.marching_cubes (gen_mesh.py:88-129) for this package's ``NeRF`` ``fn``: numpy ``(vertices float64 [V, 3],
    triangles int64 [T, 3])``. The vertices are rescaled exactly as the reference does, ``vertices * (c2 - c1) / reso + c1``:
    note that this divides by ``reso``, not ``reso - 1`` (the lattice's node spacing), so the mesh comes out shrunk by
    (reso - 1) / reso towards c1 - kept for parity with the reference."""
    c1, c2, reso = _axes(c1, c2, reso)
    sigma = density_grid(fn, c1, c2, reso, chunk)
    v, t = marching_cubes_volume(sigma, isosurface)
    vertices = v.cpu().numpy().astype(np.float64)
    c1a, c2a = np.array(c1), np.array(c2)
    vertices *= (c2a - c1a) / np.array(reso)
    return vertices + c1a, t.cpu().numpy()


def save_obj(vertices, triangles, path, vert_rgb=None):
    """Wavefront OBJ as gen_mesh.save_obj writes it (gen_mesh.py:133-158): ``v x y z`` (``%.4f``), or ``v x y z r g b``
    with ``vert_rgb``, then ``f a b c`` with 1-based vertex ids."""
    def host(a):
        return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    vertices, triangles = host(vertices), host(triangles)
    lines = []
    if vert_rgb is None:
        for v in vertices.tolist():
            lines.append("v %.4f %.4f %.4f\n" % (v[0], v[1], v[2]))
    else:
        for v, c in zip(vertices.tolist(), host(vert_rgb).tolist()):
            lines.append("v %.4f %.4f %.4f %.4f %.4f %.4f\n" % (v[0], v[1], v[2], c[0], c[1], c[2]))
    for f in (triangles.astype(np.int64) + 1).tolist():
        lines.append("f %d %d %d\n" % (f[0], f[1], f[2]))
    with open(path, "w") as fh:
        fh.write("".join(lines))
