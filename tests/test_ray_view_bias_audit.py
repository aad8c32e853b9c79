"""Static audit of nerf_mlp_h2_fold_ray_kernel (mlp_kernel_h2.hip), the folded kernel with the per-ray view bias, in its two
input modes.

In ray mode it adds one LDS-DMA per tile (the ray's row into the wave's slot) to the vector-memory counter the weight ring owns, and reads
the slot with the inline-asm reads and counted waits the bias tiles are read with; in the indexed mode each lane loads its entries from the table at the end of the tile. The checks of tests/test_view_fold_audit.py
on its assembly: no register touched before the hand-counted wait that retires its LDS read, no scalar hazard in front of an
inline-asm store, no scratch in the code and none in the compiler's resource report. CPU only."""
import importlib.util
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nerf-projects_amd")
KERNELS = ("nerf_mlp_h2_fold_ray_kernelILi2EE", "nerf_mlp_h2_fold_ray_kernelILi4EE")      # rays, indexed rays


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_ray_bias_kernel_passes_the_lds_wait_audit(tmp_path):
    build = _load(os.path.join(PKG, "build.py"), "nerf_build_for_ray_bias_audit")
    audit = _load(os.path.join(ROOT, "tools", "audit_lds_waits.py"), "audit_lds_waits")
    src = "mlp_kernel_h2.hip"
    out = tmp_path / (src + ".s")
    cmd = [build.hipcc()] + build.FLAGS + build.EXTRA.get(src, build.VGPR_FORM) + \
        ["-I", os.path.join(ROOT, "include"), "-I", build.CSRC, "--cuda-device-only", "-S",
         "-Rpass-analysis=kernel-resource-usage", os.path.join(build.CSRC, src), "-o", str(out)]
    r = subprocess.run(cmd, check=True, cwd=tmp_path, capture_output=True, text=True)
    text = open(out).read()
    for inst in KERNELS:
        findings, n_ops, n_waits = audit.audit(str(out), inst)
        # (found and parsed: the folded kernel's bars; this one is one chunk of 66 shorter)
        assert n_ops > 1000 and n_waits > 400, (n_ops, n_waits)
        assert not findings, findings[:5]
        hazards = audit.audit_sgpr_hazards(str(out), inst)
        assert not hazards, hazards[:5]
        body = text[text.index(inst):]
        body = body[:body.index("s_endpgm")]
        assert "scratch_" not in body
        assert len(re.findall(r"global_load_lds_dwordx4", body)) > 8      # (the ring's pieces and the row's LDS-DMA)
        # the build report: 0 bytes of scratch, no vector register spilled
        report = r.stderr[r.stderr.index(inst):]
        report = report[:report.index("LDS Size")  + 80]
        assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", report), report
        assert re.search(r"VGPRs Spill: 0\b", report), report
