"""The shipped kernel sources carry no compile-time switch, and build.py offers no way to pass one to the product build."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nerf-projects_amd")
CSRC = os.path.join(PKG, "csrc")


def test_no_switch_in_the_kernel_sources_and_none_through_the_build():
    for name in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, name)) as f:
            for no, line in enumerate(f, 1):
                assert not re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b.*\bNERF_", line), (name, no, line)
                assert not re.match(r"\s*#\s*define\s+NERF_FRAG_VGPR\b", line), (name, no, line)

    with open(os.path.join(PKG, "build.py")) as f:
        assert "NERF_EXTRA_FLAGS" not in f.read()

    spec = importlib.util.spec_from_file_location("nerf_build_for_switch_test", os.path.join(PKG, "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    headers = {os.path.join(CSRC, n) for n in os.listdir(CSRC) if n.endswith((".h", ".inc"))}
    assert headers and headers <= set(build.HEADERS)
    assert os.path.join(ROOT, "include", "nerf_mi355x.h") in build.HEADERS
