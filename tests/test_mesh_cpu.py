"""CPU-side checks of the mesh-extraction boundary (include/nerf_mi355x.h, "Mesh extraction"): the two argument structs match
their ctypes mirrors field by field, the entry points are bound, save_obj writes gen_mesh's text, and the lattice instantiation
of the fp16-pair kernel passes the static audit of its hand-counted LDS waits. No GPU is used."""
import ctypes
import importlib.util
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nerf_mi355x.h")
PKG = os.path.join(ROOT, "nerf-projects_amd")


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_mesh_structs_match_header(tmp_path):
    """offsetof of every field and sizeof of nerf_grid_args / nerf_mc_args from a gcc compile of the header, against ctypes."""
    from nerf_projects_amd import _lib
    pairs = [("nerf_grid_args", _lib.GridArgs), ("nerf_mc_args", _lib.McArgs)]
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "nerf_mi355x.h"', 'int main(void){']
    want = []
    for cname, ct in pairs:
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), header, flags=re.S).group(1)
        c_fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            for name in decl.split(","):                 # `double c1[3], c2[3]` / `float* sigma`
                c_fields.append(re.sub(r"\[.*\]", "", name.strip().split()[-1].lstrip("*")))
        py_fields = [f[0] for f in ct._fields_]
        assert c_fields == py_fields, f"{cname}: header fields {c_fields} != ctypes fields {py_fields}"
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        want.append(ctypes.sizeof(ct))
        for f in py_fields:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {f}));')
            want.append(getattr(ct, f).offset)
    lines.append('return 0;}')
    src = tmp_path / "mesh_fields.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "mesh_fields"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want


def test_mesh_entry_points_bound():
    from nerf_projects_amd import _lib
    assert "nerf_density_grid" in _lib.EXPORTS and "nerf_marching_cubes" in _lib.EXPORTS
    import nerf_projects_amd as N
    for name in ("density_grid", "marching_cubes_volume", "marching_cubes", "save_obj"):
        assert callable(getattr(N, name)), name


MESH_V = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.23456]], dtype=np.float64)
MESH_F = np.array([[0, 1, 2], [0, 2, 3], [3, 2, 1]], dtype=np.int64)
MESH_RGB = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.25, 0.125]], dtype=np.float64)
OBJ_PLAIN = ("v 0.0000 0.0000 0.0000\nv 1.0000 0.0000 0.0000\nv 0.0000 1.0000 0.0000\nv 0.0000 0.0000 -1.2346\n"
             "f 1 2 3\nf 1 3 4\nf 4 3 2\n")
OBJ_RGB = ("v 0.0000 0.0000 0.0000 1.0000 0.0000 0.0000\nv 1.0000 0.0000 0.0000 0.0000 1.0000 0.0000\n"
           "v 0.0000 1.0000 0.0000 0.0000 0.0000 1.0000\nv 0.0000 0.0000 -1.2346 0.5000 0.2500 0.1250\n"
           "f 1 2 3\nf 1 3 4\nf 4 3 2\n")


def test_save_obj_text(tmp_path):
    """gen_mesh.save_obj's format (gen_mesh.py:133-158): %.4f vertices, optional colours, 1-based faces."""
    from nerf_projects_amd import save_obj
    p = tmp_path / "a.obj"
    save_obj(MESH_V, MESH_F, str(p))
    assert p.read_bytes() == OBJ_PLAIN.encode()
    save_obj(MESH_V, MESH_F, str(p), vert_rgb=MESH_RGB)
    assert p.read_bytes() == OBJ_RGB.encode()


def test_lattice_kernel_lds_waits(tmp_path):
    """tools/audit_lds_waits.py on nerf_mlp_h2_kernel<kInputLattice, 0>: no register touched before its hand-counted LDS
    wait, no scalar hazard, no scratch (tests/test_kernel_audit.py covers the other instantiations)."""
    build = _load(os.path.join(PKG, "build.py"), "nerf_build_for_mesh_audit")
    audit = _load(os.path.join(ROOT, "tools", "audit_lds_waits.py"), "audit_lds_waits_mesh")
    src = "mlp_kernel_h2.hip"
    out = tmp_path / (src + ".s")
    cmd = [build.hipcc()] + build.FLAGS + build.EXTRA.get(src, build.VGPR_FORM) + \
        ["-I", os.path.join(ROOT, "include"), "-I", build.CSRC, "--cuda-device-only", "-S",
         os.path.join(build.CSRC, src), "-o", str(out)]
    subprocess.run(cmd, check=True, cwd=tmp_path)
    inst = "kernelILi3ELi0E"
    findings, n_ops, n_waits = audit.audit(str(out), inst)
    assert n_ops > 1000 and n_waits > 400, (inst, n_ops, n_waits)
    assert not findings, (inst, findings[:5])
    assert not audit.audit_sgpr_hazards(str(out), inst), inst
    text = open(out).read()
    body = text[text.index(inst):]
    body = body[:body.index("s_endpgm")]
    assert "scratch_" not in body, inst
