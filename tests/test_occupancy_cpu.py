"""Occupancy grid, CPU side: the numpy restatement of the cell rule and of grid construction (include/nerf_mi355x.h,
"Occupancy grid") against hand-made lattices, the static audit of the indexed instantiations of the fused kernels, and the
presence of the new entry points. tests/test_occupancy.py (GPU) compares the library with these functions."""
import itertools
import os
import re
import subprocess

import numpy as np

from test_kernel_audit import PKG, ROOT, _load

F32 = np.float32


# ---- the restatement ------------------------------------------------------------------------------

def np_cells(lattices, threshold=0.0, dilate=0, cell_mask=None):
    """Cells [X-1, Y-1, Z-1] from sigma lattices [X, Y, Z]: a cell is occupied when sigma at any of its 8 corner nodes is
    > threshold or NaN in any lattice (or its entry of cell_mask is set), grown `dilate` times by one cell in all 26
    directions."""
    occ = None if cell_mask is None else np.asarray(cell_mask) != 0
    for s in lattices:
        s = np.asarray(s, F32)
        hit = (s > F32(threshold)) | np.isnan(s)
        X, Y, Z = s.shape
        c = np.zeros((X - 1, Y - 1, Z - 1), bool)
        for di, dj, dk in itertools.product((0, 1), repeat=3):
            c |= hit[di:X - 1 + di, dj:Y - 1 + dj, dk:Z - 1 + dk]
        occ = c if occ is None else occ | c
    for _ in range(dilate):
        p = np.pad(occ, 1)
        grown = np.zeros_like(occ)
        for di, dj, dk in itertools.product((0, 1, 2), repeat=3):
            grown |= p[di:di + occ.shape[0], dj:dj + occ.shape[1], dk:dk + occ.shape[2]]
        occ = grown
    return occ


def np_cell_index(pts, cells_shape, c1, c2):
    """(inside [..], idx [.., 3]) of fp32 points: inside iff c1 <= p <= c2 on every axis; the index on an axis is
    min(floor((p - c1) / cell), n_cells - 1) with cell = (c2 - c1) / n_cells, every operation rounded to fp32."""
    pts = np.asarray(pts, F32)
    c1f, c2f = np.broadcast_to(np.asarray(c1, F32), (3,)), np.broadcast_to(np.asarray(c2, F32), (3,))
    nc = np.asarray(cells_shape, np.int64)
    cell = ((c2f - c1f) / nc.astype(F32)).astype(F32)
    with np.errstate(invalid="ignore"):
        inside = ((pts >= c1f) & (pts <= c2f)).all(-1)
        t = ((pts - c1f).astype(F32) / cell).astype(F32)
    t = np.where(inside[..., None], t, F32(0))
    idx = np.minimum(np.floor(t).astype(np.int64), nc - 1)
    return inside, idx


def np_keep(pts, cells, c1, c2, outside="evaluate"):
    """keep [N, S] of pts [N, S, 3]: the last sample of every ray, occupied cells, non-finite positions, and points outside
    the box when outside == "evaluate"."""
    pts = np.asarray(pts, F32)
    inside, idx = np_cell_index(pts, cells.shape, c1, c2)
    finite = np.isfinite(pts).all(-1)
    keep = np.where(inside, cells[idx[..., 0], idx[..., 1], idx[..., 2]], outside == "evaluate")
    keep = keep | ~finite
    keep[..., -1] = True
    return keep


# ---- the restatement against hand-made cases ------------------------------------------------------

def test_eight_corner_rule_and_nan_node():
    s = np.full((4, 5, 6), -1.0, F32)
    s[1, 2, 3] = 0.5                      # one node above the threshold: the 8 cells around it
    want = np.zeros((3, 4, 5), bool)
    want[0:2, 1:3, 2:4] = True
    assert np.array_equal(np_cells([s]), want)
    s[1, 2, 3] = 0.0                      # sigma > threshold is strict
    assert not np_cells([s]).any()
    assert np.array_equal(np_cells([s], threshold=-0.5), want)
    s[3, 4, 5] = np.nan                   # a NaN node counts as occupied: the corner node touches one cell
    c = np_cells([s])
    assert c.sum() == 1 and c[2, 3, 4]
    # two lattices: the union
    t = np.full((4, 5, 6), -1.0, F32)
    t[0, 0, 0] = 1.0
    c2 = np_cells([s, t])
    assert c2.sum() == 2 and c2[0, 0, 0] and c2[2, 3, 4]


def test_dilate_rounds():
    m = np.zeros((7, 7, 7), bool)
    m[3, 3, 3] = True
    for d, side in ((0, 1), (1, 3), (2, 5)):
        c = np_cells([], dilate=d, cell_mask=m)
        assert c.sum() == side ** 3 and c[3 - d:4 + d, 3 - d:4 + d, 3 - d:4 + d].all(), d
    m[:] = False
    m[0, 0, 6] = True                     # growth stops at the faces of the box
    assert np_cells([], dilate=1, cell_mask=m).sum() == 8
    assert np_cells([], dilate=7, cell_mask=m).all()


def test_upper_faces_and_outside_modes():
    cells = np.zeros((4, 4, 4), bool)
    cells[3, 3, 3] = True
    cells[0, 0, 0] = True
    c1, c2 = -1.0, 1.0                    # cell size 0.5
    pts = np.array([[[1.0, 1.0, 1.0],     # the upper corner: last cell
                     [-1.0, -1.0, -1.0],  # the lower corner: first cell
                     [0.5, 0.5, 0.5],     # a node: the cell above it
                     [0.49, 0.6, 0.6],    # x in cell 2: empty
                     [1.0000001, 0.9, 0.9],   # just outside
                     [np.nan, 0.0, 0.0],
                     [0.0, np.inf, 0.0],
                     [0.0, 0.0, 0.0]]], F32)      # last sample: always kept
    inside, idx = np_cell_index(pts, cells.shape, c1, c2)
    assert inside[0].tolist() == [True, True, True, True, False, False, False, True]
    assert idx[0, 0].tolist() == [3, 3, 3] and idx[0, 1].tolist() == [0, 0, 0] and idx[0, 2].tolist() == [3, 3, 3]
    assert idx[0, 3].tolist() == [2, 3, 3]
    assert np_keep(pts, cells, c1, c2, "evaluate")[0].tolist() == [True, True, True, False, True, True, True, True]
    assert np_keep(pts, cells, c1, c2, "empty")[0].tolist() == [True, True, True, False, False, True, True, True]
    # an empty grid keeps the last samples only
    assert np_keep(pts, np.zeros_like(cells), c1, c2, "empty")[0].tolist() == [False] * 5 + [True] * 3


# ---- the kernels and the entry points --------------------------------------------------------------

def _device_asm(src, tmp_path):
    build = _load(os.path.join(PKG, "build.py"), "nerf_build_for_audit")
    out = tmp_path / (src + ".s")
    cmd = [build.hipcc()] + build.FLAGS + build.EXTRA.get(src, build.VGPR_FORM) + \
        ["-I", os.path.join(ROOT, "include"), "-I", build.CSRC, "--cuda-device-only", "-S",
         os.path.join(build.CSRC, src), "-o", str(out)]
    subprocess.run(cmd, check=True, cwd=tmp_path)
    return str(out)


def _body(text, inst):
    body = text[text.index(inst):]
    return body[:body.index("s_endpgm")]


def test_indexed_kernels_pass_the_audit(tmp_path):
    """The kInputRaysIndexed instantiations obey the rules tests/test_kernel_audit.py enforces for the others: no register
    touched before the wait that retires its LDS read, no scalar hazard in front of an inline-asm store, no scratch."""
    audit = _load(os.path.join(ROOT, "tools", "audit_lds_waits.py"), "audit_lds_waits")
    out = _device_asm("mlp_kernel_h2.hip", tmp_path)
    inst = "kernelILi4ELi0E"
    findings, n_ops, n_waits = audit.audit(out, inst)
    assert n_ops > 1000 and n_waits > 400, (n_ops, n_waits)
    assert not findings, findings[:5]
    assert not audit.audit_sgpr_hazards(out, inst)
    text = open(out).read()
    assert "scratch_" not in _body(text, inst)
    # the list's length is one scalar load, not a per-lane value carried through the layers
    assert re.search(r"s_load_dword\b", _body(text, inst))
    out32 = _device_asm("mlp_kernel.hip", tmp_path)
    assert "scratch_" not in _body(open(out32).read(), "nerf_mlp_kernelILi4ELb0E")
    assert not audit.audit_sgpr_hazards(out32, "nerf_mlp_kernelILi4ELb0E")


def test_no_workgroup_waits_for_another():
    """The compaction is three plain launches: no spin-wait, no atomic append (the only atomic is the cell count)."""
    src = open(os.path.join(PKG, "csrc", "occupancy_kernels.hip")).read()
    code = re.sub(r"//.*", "", src)
    assert "while" not in code and "__threadfence" not in code and "volatile" not in code
    assert code.count("atomic") == 1 and "atomicAdd(n_occupied" in code


def test_entry_points_are_declared_and_exported():
    from nerf_projects_amd import _lib
    header = open(os.path.join(ROOT, "include", "nerf_mi355x.h")).read()
    names = ("nerf_occupancy_create", "nerf_occupancy_destroy", "nerf_occupancy_cells", "nerf_occupancy_stats",
             "nerf_render_rays_occ", "nerf_render_frame_occ")
    if not os.path.exists(_lib.library_path()):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert n in _lib.EXPORTS and hasattr(lib, n), n
    assert "Occupancy grid" in header and "NERF_OCC_EVALUATE" in header and "NERF_OCC_EMPTY" in header
    import nerf_projects_amd as pkg
    assert hasattr(pkg, "OccupancyGrid")
    import inspect
    assert list(inspect.signature(pkg.render_rays).parameters)[-1] == "occupancy"
