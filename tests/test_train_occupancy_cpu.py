"""Training with an occupancy grid, CPU side: the two new entries of the C ABI (declared, bound, exported, their argument
checks), the self-checks of tests/golden/train_occupancy.npz, and the static audit of the new kInputRaysIndexed STORE
instantiations of the fused kernels. tests/test_train_occupancy.py (GPU) runs the step. No GPU is used."""
import ctypes as C
import os
import re

import numpy as np

from conftest import load_golden
from test_kernel_audit import PKG, ROOT, _load
from test_occupancy_cpu import _body, np_keep

NEW = ("nerf_train_step_occ", "nerf_occupancy_refresh")
CASES = ("ball_eval", "ball_empty", "checker_eval", "checker_empty", "empty", "full", "ball_empty_noise")


class FakeGrid(C.Structure):
    """The head of struct nerf_occupancy (csrc/ctx_internal.h) as far as the argument checks read it: the owning context
    and the box / resolution of OccGrid. Filled by hand: every refusal below comes before anything else is dereferenced."""
    _fields_ = [("ctx", C.c_void_p), ("bits", C.c_void_p), ("c1", C.c_float * 3), ("c2", C.c_float * 3), ("cell", C.c_float * 3),
                ("nc", C.c_int32 * 3), ("wz", C.c_int32), ("outside_keep", C.c_int32), ("d_bits", C.c_void_p),
                ("d_stats", C.c_void_p), ("h_stats", C.c_void_p), ("n_occupied", C.c_int64)]


def _lib():
    import nerf_projects_amd  # noqa: F401
    from nerf_projects_amd import _lib
    if not os.path.exists(_lib.library_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _lib, _lib.load()


def test_new_entries_are_declared_bound_and_exported(tmp_path):
    import subprocess
    _lib_mod, lib = _lib()
    header = open(os.path.join(ROOT, "include", "nerf_mi355x.h")).read()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert n in _lib_mod.EXPORTS and hasattr(lib, n), n
    assert lib.nerf_train_step_occ.argtypes[1]._type_ is _lib_mod.TrainArgs
    assert lib.nerf_occupancy_refresh.argtypes[1]._type_ is _lib_mod.OccupancyArgs
    # the declarations compile as C, and the two argument structs they take keep the layout of their ctypes mirrors
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "nerf_mi355x.h"',
             'int (*p_step)(nerf_ctx*, const nerf_train_args*, nerf_occupancy*) = nerf_train_step_occ;',
             'int (*p_refresh)(nerf_occupancy*, const nerf_occupancy_args*) = nerf_occupancy_refresh;', 'int main(void){']
    want = []
    for cname, ct in (("nerf_train_args", _lib_mod.TrainArgs), ("nerf_occupancy_args", _lib_mod.OccupancyArgs)):
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        want.append(C.sizeof(ct))
        for f, _ in ct._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {f}));')
            want.append(getattr(ct, f).offset)
    lines.append('return 0;}')
    src = tmp_path / "occ_train_fields.c"
    src.write_text("\n".join(lines) + "\n")
    obj = tmp_path / "occ_train_fields.o"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(obj)], check=True)
    exe = tmp_path / "occ_train_fields"
    stub = tmp_path / "stub.c"
    stub.write_text('#include "nerf_mi355x.h"\nint nerf_train_step_occ(nerf_ctx* c, const nerf_train_args* a, nerf_occupancy* o)'
                    '{(void)c;(void)a;(void)o;return 0;}\nint nerf_occupancy_refresh(nerf_occupancy* o, const nerf_occupancy_args* a)'
                    '{(void)o;(void)a;return 0;}\n')
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(obj), str(stub), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want
    import inspect
    import nerf_projects_amd as pkg
    assert "occupancy" in inspect.signature(pkg.train_on_batch).parameters
    assert callable(pkg.OccupancyGrid.refresh)


def test_argument_checks_come_before_any_device_call():
    _lib_mod, lib = _lib()
    err = lambda: lib.nerf_last_error().decode()      # noqa: E731
    fake_ctx, other_ctx = C.c_void_p(0x1000), 0x2000
    a = _lib_mod.TrainArgs()
    # nerf_train_step_occ: a NULL grid, a grid of another context
    assert lib.nerf_train_step_occ(fake_ctx, C.byref(a), None) == -1 and "NULL" in err()
    g = FakeGrid()
    g.ctx = other_ctx
    assert lib.nerf_train_step_occ(fake_ctx, C.byref(a), C.cast(C.pointer(g), C.c_void_p)) == -1 and "another context" in err()
    assert lib.nerf_train_step_occ(None, C.byref(a), C.cast(C.pointer(g), C.c_void_p)) == -1 and "another context" in err()
    # nerf_occupancy_refresh: NULL arguments, another resolution, another box, no lattice, bad scalars
    g = FakeGrid()
    g.c1[:], g.c2[:], g.nc[:] = (-1.5,) * 3, (1.5,) * 3, (16,) * 3
    gp = C.cast(C.pointer(g), C.c_void_p)

    def args(**kw):
        r = _lib_mod.OccupancyArgs()
        r.c1[:], r.c2[:], r.reso[:] = (-1.5,) * 3, (1.5,) * 3, (17,) * 3
        r.n_lattices, r.cell_mask, r.dilate, r.outside = 0, 0x3000, 1, _lib_mod.NERF_OCC_EMPTY
        for k, v in kw.items():
            if k in ("c1", "c2", "reso"):
                getattr(r, k)[:] = v
            else:
                setattr(r, k, v)
        return r

    assert lib.nerf_occupancy_refresh(None, C.byref(args())) == -1 and "NULL" in err()
    assert lib.nerf_occupancy_refresh(gp, None) == -1 and "NULL" in err()
    for kw, word in ((dict(reso=(17, 17, 33)), "keeps box and resolution"), (dict(reso=(9, 9, 9)), "keeps box and resolution"),
                     (dict(c2=(1.5, 1.5, 2.0)), "keeps box and resolution"), (dict(c1=(-1.0, -1.5, -1.5)), "keeps box and resolution"),
                     (dict(cell_mask=0), "required"), (dict(n_lattices=9), "required"), (dict(dilate=-1), "dilate"),
                     (dict(outside=7), "outside"), (dict(threshold=float("nan")), "threshold")):
        assert lib.nerf_occupancy_refresh(gp, C.byref(args(**kw))) == -1 and word in err(), (kw, err())
    # everything in order but the handle is not a live grid (no context): still refused before any device call
    assert lib.nerf_occupancy_refresh(gp, C.byref(args())) == -1 and "no context" in err()


def test_fixture_self_checks():
    g = load_golden("train_occupancy")
    n, sc, si, nc = len(g["rays"]), int(g["n_samples"]), int(g["n_importance"]), int(g["reso"]) - 1
    assert (n, sc, si) == (48, 16, 32) and g["rays"].shape == (48, 11) and g["target"].shape == (48, 3)
    c1, c2, eps = float(g["c1"]), float(g["c2"]), float(g["face_eps"])
    assert eps == 1e-4 and int(g["redrawn"]) >= 0
    cells = {k: np.unpackbits(g[f"mask.{k}"])[:nc ** 3].reshape(nc, nc, nc).astype(bool) for k in ("ball", "checker", "empty", "full")}
    assert cells["full"].all() and not cells["empty"].any()
    i, j, k = np.indices((nc,) * 3)
    assert np.array_equal(cells["checker"], (i + j + k) % 2 == 0)
    assert cells["ball"][nc // 2, nc // 2, nc // 2] and not cells["ball"][0, 0, 0]
    rays = g["rays"]
    for name in CASES:
        mask, outside = str(g[f"{name}.mask"]), str(g[f"{name}.outside"])
        z = g[f"{name}.z_fine"]
        assert z.shape == (n, sc + si) and (np.diff(z, axis=-1) >= 0).all()
        # no fine sample within face_eps of a face, and the recorded keep bits are np_keep's of the recorded depths
        pts = (rays[:, None, 0:3] + (rays[:, None, 3:6] * z[..., None]).astype(np.float32)).astype(np.float32)
        t = (pts.astype(np.float64) - c1) / ((c2 - c1) / nc)
        d = np.abs(t - np.round(t))
        assert not ((d < eps) & (t > -1.0) & (t < nc + 1.0)).any(), name
        keep = np_keep(pts, cells[mask], c1, c2, outside)
        assert np.array_equal(keep.reshape(-1), np.unpackbits(g[f"{name}.keep_f"])[:keep.size].astype(bool)), name
        kc, kf = int(g[f"{name}.kept_c"]), int(g[f"{name}.kept_f"])
        assert kf == keep.sum() and kc == np.unpackbits(g[f"{name}.keep_c"])[:n * sc].sum()
        assert abs(float(g[f"{name}.kept_fraction"]) - (kc + kf) / (n * (2 * sc + si))) < 1e-12
        # the reference's fp32 and fp64 runs: finite, and a hair apart
        for key in ("img_loss", "img_loss0"):
            a, b = float(g[f"{name}.{key}"]), float(g[f"{name}.{key}.f64"])
            assert np.isfinite(a) and np.isfinite(b) and abs(a - b) < 1e-5, (name, key, a, b)
        for tag in ("c", "f"):
            assert np.isfinite(g[f"{name}.ggap_{tag}"]).all() and np.isfinite(g[f"{name}.gnorm_{tag}.f64"]).all()
            assert np.isfinite(float(g[f"{name}.wgap_rms_{tag}"]))
            if mask != "full":
                assert len(g[f"{name}.gsub_{tag}"]) == g[f"gsub_len_{tag}"].sum() and len(g[f"{name}.wsub_{tag}"]) == g[f"wsub_len_{tag}"].sum()
    assert 0.3 <= float(g["ball_empty.kept_fraction"]) <= 0.5
    assert int(g["empty.kept_c"]) == int(g["empty.kept_f"]) == n          # only the forced last samples: M = 48 < 64
    assert float(g["full.kept_fraction"]) == 1.0
    assert float(g["checker_empty.kept_fraction"]) < float(g["checker_eval.kept_fraction"]) < 1.0
    # skipping changes the result (the masks are not vacuous), and the noise case differs from the plain one
    assert abs(float(g["ball_empty.img_loss"]) - float(g["full.img_loss"])) > 1e-3
    assert abs(float(g["ball_empty_noise.img_loss"]) - float(g["ball_empty.img_loss"])) > 1e-4
    # the loop
    it = int(g["loop.n_iters"])
    assert it == 20 and len(g["loop.img_loss"]) == it and float(g["loop.closest_face"]) >= 5e-6
    for key in ("img_loss", "img_loss0"):
        a, b = g[f"loop.{key}"], g[f"loop.{key}.f64"]
        assert np.isfinite(a).all() and np.isfinite(b).all() and np.abs(a - b).max() < 1e-4
    assert g["loop.img_loss"][-1] < 0.5 * g["loop.img_loss"][0]          # it trains
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "train_occupancy.npz")) < 768 * 1024


def test_mask_iv_is_the_unmasked_step():
    """The masked reference under an all-occupied mask is the reference's plain loop body on the same inputs: bit for bit
    (multiplying by a mask of ones and adding no noise changes nothing)."""
    g = load_golden("train_occupancy")
    assert float(g["full.img_loss"]) == float(g["unmasked.img_loss"]) and float(g["full.img_loss0"]) == float(g["unmasked.img_loss0"])
    assert np.array_equal(g["full.rgb"], g["unmasked.rgb"])
    for tag in ("c", "f"):
        assert np.array_equal(g[f"full.gnorm_{tag}"], g[f"unmasked.gnorm_{tag}"])


def test_new_instantiations_pass_the_audit_and_use_no_scratch(tmp_path):
    """nerf_mlp_h2_kernel<kInputRaysIndexed, 1 | 2> and nerf_mlp_kernel<kInputRaysIndexed, true>: the LDS-wait audit and the
    scalar-hazard audit of tools/audit_lds_waits.py as tests/test_occupancy_cpu.py calls them for the inference kernels, no
    scratch in the code, and the compiler's resource remark says the same."""
    import subprocess
    audit = _load(os.path.join(ROOT, "tools", "audit_lds_waits.py"), "audit_lds_waits")
    build = _load(os.path.join(PKG, "build.py"), "nerf_build_for_remarks")

    def asm_and_remarks(src):      # (_device_asm of tests/test_occupancy_cpu.py with the resource remarks: one compile for both)
        out = tmp_path / (src + ".s")
        cmd = [build.hipcc()] + build.FLAGS + build.EXTRA.get(src, build.VGPR_FORM) + \
            ["-I", os.path.join(ROOT, "include"), "-I", build.CSRC, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
             "-S", os.path.join(build.CSRC, src), "-o", str(out)]
        return str(out), subprocess.run(cmd, check=True, cwd=tmp_path, capture_output=True, text=True).stderr

    def no_scratch_remark(remarks, inst):
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", remarks[remarks.index(inst):])
        assert m and int(m.group(1)) == 0, (inst, m and m.group(0))

    out, remarks = asm_and_remarks("mlp_kernel_h2.hip")
    text = open(out).read()
    for inst in ("kernelILi4ELi1E", "kernelILi4ELi2E"):
        findings, n_ops, n_waits = audit.audit(out, inst)
        assert n_ops > 1000 and n_waits > 400, (inst, n_ops, n_waits)
        assert not findings, (inst, findings[:5])
        assert not audit.audit_sgpr_hazards(out, inst), inst
        assert "scratch_" not in _body(text, inst), inst
        assert re.search(r"s_load_dword\b", _body(text, inst)), inst      # the list's length: one scalar load
        no_scratch_remark(remarks, "nerf_mlp_h2_" + inst)
    out32, remarks32 = asm_and_remarks("mlp_kernel.hip")
    assert "scratch_" not in _body(open(out32).read(), "nerf_mlp_kernelILi4ELb1E")
    assert not audit.audit_sgpr_hazards(out32, "nerf_mlp_kernelILi4ELb1E")
    no_scratch_remark(remarks32, "nerf_mlp_kernelILi4ELb1E")
