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


def test_the_library_reads_six_environment_switches_once_each():
    """The run-time switches of the library are the three that bench.py, bench_train.py and the public header name and the
    three reference routes of test_train_glue_is_bit_identical; each is read by one getenv call, and no getenv takes a name
    that is not spelled out at the call."""
    kept = {"NERF_TRAIN_FORWARD", "NERF_TRAIN_BWD", "NERF_TRAIN_DW", "NERF_TRAIN_GLUE", "NERF_TRAIN_BLOCKED", "NERF_TRAIN_NARROW"}
    names, calls = [], 0
    for name in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        calls += len(re.findall(r"\bgetenv\s*\(", text))
        names += re.findall(r"\bgetenv\s*\(\s*\"(NERF_[A-Za-z0-9_]*)\"\s*\)", text)
    assert sorted(names) == sorted(kept), sorted(names)
    assert calls == len(names), (calls, names)
