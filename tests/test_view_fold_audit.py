"""Static audit of the folded inference kernel, nerf_mlp_h2_fold_kernel<MODE> (mlp_kernel_h2.hip).

The folded kernel is a kernel of its own because a run-time fold flag inside nerf_mlp_h2_kernel spilled to scratch, and it
is the kernel that renders every eligible view-dependent network, the benchmark's included. tests/test_kernel_audit.py
selects nerf_mlp_h2_kernel's instantiations by name, so the five input modes of the folded twin get the same checks here:
no register touched before the hand-counted wait that retires its LDS read, no scalar hazard in front of an inline-asm
store, and no scratch (a reload would go through the vector-memory counter the weight ring owns). CPU only."""
import importlib.util
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nerf-projects_amd")

# embedded rows, points, rays, lattice, indexed rays
FOLD_KERNELS = tuple(f"nerf_mlp_h2_fold_kernelILi{mode}EE" for mode in range(5))


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_folded_kernels_pass_the_lds_wait_audit(tmp_path):
    build = _load(os.path.join(PKG, "build.py"), "nerf_build_for_fold_audit")
    audit = _load(os.path.join(ROOT, "tools", "audit_lds_waits.py"), "audit_lds_waits")
    src = "mlp_kernel_h2.hip"
    out = tmp_path / (src + ".s")
    cmd = [build.hipcc()] + build.FLAGS + build.EXTRA.get(src, build.VGPR_FORM) + \
        ["-I", os.path.join(ROOT, "include"), "-I", build.CSRC, "--cuda-device-only", "-S",
         os.path.join(build.CSRC, src), "-o", str(out)]
    subprocess.run(cmd, check=True, cwd=tmp_path)
    text = open(out).read()
    for inst in FOLD_KERNELS:
        findings, n_ops, n_waits = audit.audit(str(out), inst)
        # (the bars tests/test_kernel_audit.py uses to know that the unfolded kernel was found and parsed; the folded one is
        # 8 chunks of 74 shorter and well above them)
        assert n_ops > 1000 and n_waits > 400, (inst, n_ops, n_waits)
        assert not findings, (inst, findings[:5])
        hazards = audit.audit_sgpr_hazards(str(out), inst)
        assert not hazards, (inst, hazards[:5])
        body = text[text.index(inst):]
        body = body[:body.index("s_endpgm")]
        assert "scratch_" not in body, inst
