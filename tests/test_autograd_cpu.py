"""CPU-side checks of the taped route's ABI (nerf_train_forward / nerf_train_backward / nerf_zero_grad / nerf_adam_step):
the entry points are bound, every field of the two new argument structs matches a C compile of the header, and the
structs carry their own size. No compute calls are made here."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nerf_mi355x.h")
NEW = ("nerf_train_forward", "nerf_train_backward", "nerf_zero_grad", "nerf_adam_step")


@pytest.fixture(scope="module")
def lib():
    from nerf_projects_amd import _lib
    if not os.path.exists(_lib.library_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_entry_points_bound(lib):
    from nerf_projects_amd import _lib
    for name in NEW:
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
        assert getattr(lib, name).restype is ctypes.c_int


def test_struct_fields_match_header(lib, tmp_path):
    """offsetof of every field and sizeof of nerf_train_forward_args / nerf_train_backward_args against the ctypes mirror."""
    from nerf_projects_amd import _lib
    pairs = [("nerf_train_forward_args", _lib.TrainForwardArgs), ("nerf_train_backward_args", _lib.TrainBackwardArgs)]
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
            for name in decl.split(","):
                c_fields.append(re.sub(r"\[.*\]", "", name.strip().split()[-1].lstrip("*")))
        py_fields = [f[0] for f in ct._fields_]
        assert c_fields == py_fields, f"{cname}: header fields {c_fields} != ctypes fields {py_fields}"
        assert py_fields[0] == "struct_size"
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        want.append(ctypes.sizeof(ct))
        for f in py_fields:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {f}));')
            want.append(getattr(ct, f).offset)
    lines.append('return 0;}')
    src = tmp_path / "fields.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "fields"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want


def test_structs_carry_their_size(lib):
    from nerf_projects_amd import _lib
    assert _lib.TrainForwardArgs().struct_size == ctypes.sizeof(_lib.TrainForwardArgs)
    assert _lib.TrainBackwardArgs().struct_size == ctypes.sizeof(_lib.TrainBackwardArgs)


def test_calls_without_a_context_are_refused(lib):
    """NULL context or arguments: NERF_E_INVALID and a message, before anything touches a device."""
    from nerf_projects_amd import _lib
    f, b = _lib.TrainForwardArgs(), _lib.TrainBackwardArgs()
    assert lib.nerf_train_forward(None, ctypes.byref(f)) == -1
    assert lib.nerf_train_backward(None, ctypes.byref(b)) == -1
    assert lib.nerf_zero_grad(None, 0, None) == -1
    slots = (ctypes.c_int32 * 1)(0)
    assert lib.nerf_adam_step(None, slots, 1, 1e-3, 0.9, 0.999, 1e-8, 1, None) == -1
    assert len(lib.nerf_last_error()) > 0


def test_autograd_entry_points_on_the_package():
    """NeRF.requires_grad_ exists, as on nn.Module, and Adam has step() and zero_grad(). (That requires_grad is off on a
    new model is checked on the GPU, tests/test_autograd.py: constructing a model needs one.)"""
    import nerf_projects_amd as N
    assert callable(N.NeRF.requires_grad_)
    assert callable(N.Adam.step) and callable(N.Adam.zero_grad)
