"""PlenOctree's backward without a GPU (include/nerf_mi355x.h, "PlenOctree: backward"): the gradient oracle's march against
``octree_oracle.march`` bit for bit, its fp64 backward against central differences of that march, what the dense cases add
(rays that stop, channels outside [0, 1]), a descent step, the container's new surface, the struct mirror and the generated
code of the backward kernels."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import octree_grad_oracle as G  # noqa: E402
import octree_oracle as O  # noqa: E402
from grid_testlib import assert_structs_match_c_header, compile_kernels_to_asm  # noqa: E402

ALL_CASES = sorted(O.CASES) + sorted(G.DENSE)


@pytest.fixture(scope="module")
def N():
    import nerf_projects_amd
    return nerf_projects_amd


def options(thresh, bg):
    return dict(step_size=1e-3, sigma_thresh=thresh, stop_thresh=thresh, background_brightness=bg)


# ---- 1. the recording march is the oracle's march ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES)
def test_recording_march_equals_the_oracle_march(name):
    _, t, o, d = G.case(name)
    for rad in (np.float32, np.float64):
        for thresh, bg in ((0.0, 1.0), (1e-2, 0.5)):
            want = O.march(t, o, d, rad=rad, **options(thresh, bg))
            got = G.march(t, o, d, rad=rad, **options(thresh, bg))
            assert got[0].dtype == want[0].dtype and np.array_equal(got[0], want[0], equal_nan=True)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
            assert got[3].shape == got[2].shape and ((got[3] > 0) == (got[2] >= 0)).all()      # a len for every leaf


# ---- 2. the fp64 backward against central differences ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["r8", "r16", "r8x8", "r16x8"])
def test_backward_against_central_differences(name):
    """d/d eps of sum(rgb * g) along a random direction over the touched entries, eps 1e-6, on the last 128 rays of the case
    (the special rays among them): the relative difference is at most 1e-6 (measured: at most 7e-8)."""
    _, t, o, d = G.case(name)
    o, d = o[-128:], d[-128:]
    D = t["data"].shape[-1]
    rng = np.random.default_rng(5)
    g = rng.standard_normal((o.shape[0], 3))
    worst = 0.0
    for act in ("relu_half", "sigmoid"):
        tree = O.with_activation(t, act)
        data64 = tree["data"].astype(np.float64)
        for thresh in (0.0, 1e-2):
            for bg in (1.0, 0.5):
                kw = options(thresh, bg)
                _, grad, _, _ = G.backward(tree, o, d, g=g, data=data64, **kw)
                v = rng.standard_normal(grad.shape) * (grad != 0)
                assert np.count_nonzero(v) > 100

                def f(e):
                    t2 = dict(tree)
                    t2["data"] = data64 + e * v.reshape(data64.shape)
                    return np.nansum(O.march(t2, o, d, rad=np.float64, **kw)[0] * g)

                eps = 1e-6
                fd = (f(eps) - f(-eps)) / (2 * eps)
                an = (grad * v).sum()
                rel = abs(fd - an) / abs(an)
                print(f"{name} {act} thresh {thresh} bg {bg}: fd {fd:.9g} analytic {an:.9g} rel {rel:.2e}")
                worst = max(worst, rel)
    assert worst <= 1e-6


# ---- 3. what the dense cases add --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(G.DENSE))
def test_dense_cases_stop_rays_and_leave_the_unit_interval(name):
    _, t, o, d = G.case(name)
    kw = options(1e-2, 1.0)
    g = np.ones((o.shape[0], 3))
    rgb32, steps32, _, _ = G.march(t, o, d, rad=np.float32, **kw)
    rgb64, grad, _, stopped = G.backward(t, o, d, g=g, **kw)
    steps64 = G.march(t, o, d, rad=np.float64, **kw)[1]
    print(f"{name}: {int(stopped.sum())} of {len(o)} rays stop")
    assert stopped.sum() >= len(o) // 2
    assert np.array_equal(steps32, steps64)
    relu = O.with_activation(t, "relu_half")
    out = G.march(relu, o, d, rad=np.float64, **kw)[0]
    outside = ((out < 0) | (out > 1)).any(1)
    print(f"{name}: {int(outside.sum())} rays have a channel outside [0, 1]")
    assert outside.sum() >= 1


# ---- 4. a descent step --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["r8", "r8x8", "r16"])
def test_descent_step_lowers_the_loss_by_the_first_order_amount(name):
    """L = the clamped MSE against a seeded random target; one step of lr = 1e-2 L0 / |grad|^2 along -grad lowers it by
    lr |grad|^2 to first order: the ratio lies in [0.97, 1.01]."""
    _, t, o, d = G.case(name)
    kw = options(1e-2, 1.0)
    gt = np.random.default_rng(11).random((o.shape[0], 3))
    data64 = t["data"].astype(np.float64)

    def loss(data):
        t2 = dict(t)
        t2["data"] = data
        return G.clamped_mse(O.march(t2, o, d, rad=np.float64, **kw)[0], gt)

    L0, g = loss(data64)
    _, grad, lsum, _ = G.backward(t, o, d, g=g, data=data64, **kw)
    _, fused, lsum, _ = G.backward(t, o, d, rgb_gt=gt, loss_scale=2.0 / (3 * len(o)), data=data64, **kw)
    assert np.allclose(fused, grad, rtol=1e-12, atol=0) and abs(lsum / (3 * len(o)) - L0) <= 1e-12 * L0      # the fused form
    g2 = (grad * grad).sum()
    lr = 1e-2 * L0 / g2
    L1, _ = loss(data64 - lr * grad.reshape(data64.shape))
    ratio = (L0 - L1) / (lr * g2)
    print(f"{name}: L0 {L0:.6g} L1 {L1:.6g} ratio {ratio:.4f}")
    assert 0.97 <= ratio <= 1.01


# ---- 5. the container ----------------------------------------------------------------------------------------------------------
def test_container_parameters_clone_and_save(N, tmp_path):
    _, t, o, d = O.case("r8")
    tree = N.N3Tree(t["child"], t["data"], t["parent_depth"], t["invradius"], t["offset"], "SH4", "relu_half", device="cpu")
    assert tree.parameters() == [tree.data] and tree.parameters()[0] is tree.data and not tree.data.requires_grad
    assert tree.requires_grad_() is tree and tree.data.requires_grad
    torch.optim.SGD(tree.parameters(), lr=1e7)
    torch.optim.Adam(tree.parameters(), lr=1e-2, eps=1e-8)
    c = tree.clone()
    assert c.data.requires_grad and c.data.is_leaf and c.data.grad_fn is None
    assert torch.equal(c.data, tree.data) and torch.equal(c.child, tree.child) and torch.equal(c.parent_depth, tree.parent_depth)
    assert c.data.data_ptr() != tree.data.data_ptr() and c.child.data_ptr() != tree.child.data_ptr()
    assert c.max_depth == tree.max_depth and c.rgb_activation == "relu_half" and torch.equal(c.invradius, tree.invradius)
    assert c.clone(device="cpu").device.type == "cpu"
    with torch.no_grad():
        c.data.mul_(2.0)
    assert not torch.equal(c.data, tree.data)
    path = str(tmp_path / "grad_tree.npz")
    tree.save(path)      # a tree that requires grad saves (detached)
    back = N.N3Tree.load(path, device="cpu")
    assert torch.equal(back.data, tree.data.detach().to(torch.float16).to(torch.float32)) and not back.data.requires_grad
    assert tree.requires_grad_(False) is tree and not tree.data.requires_grad and not tree.clone().data.requires_grad
    # no CPU fallback: the fused step and a differentiable render name it; rays that require grad are refused first
    tree.requires_grad_()
    rays = N.Rays(torch.from_numpy(o[:8]), torch.from_numpy(d[:8]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tree.mse_backward(rays, torch.zeros(8, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tree.volume_render(rays)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tree.volume_render_image(N.Camera(torch.eye(4)[:3], fx=10.0, width=4, height=4))
    grad_rays = N.Rays(torch.from_numpy(o[:8]).requires_grad_(), torch.from_numpy(d[:8]))
    for t2 in (tree, tree.clone().requires_grad_(False)):
        with pytest.raises(NotImplementedError, match="rays"):
            t2.volume_render(grad_rays)
        with pytest.raises(NotImplementedError, match="rays"):
            t2.mse_backward(grad_rays, torch.zeros(8, 3))


# ---- the C layer, without a device -------------------------------------------------------------------------------------------
def test_backward_struct_matches_a_c_compile_of_the_header(tmp_path):
    assert_structs_match_c_header(tmp_path, {"nerf_octree_backward_args": "OctreeBackwardArgs"})


def test_backward_entries_refuse_without_a_device():
    import ctypes as C
    from nerf_projects_amd import _lib
    lib = _lib.load()
    err = lambda: lib.nerf_last_error().decode()      # noqa: E731
    fake, ptr = C.c_void_p(0x1000), 0x2000      # never dereferenced: these checks come before the first use of a handle
    for s in ("nerf_octree_backward_rays", "nerf_octree_backward_image"):
        assert hasattr(lib, s) and s in _lib.EXPORTS

    def args(**k):
        a = _lib.OctreeBackwardArgs()
        a.origins, a.dirs, a.n_rays, a.grad_rgb, a.grad_data = ptr, ptr, 4, ptr, ptr
        for name, v in k.items():
            setattr(a, name, v)
        return a

    op = _lib.OctreeRenderOptions()
    op.step_size, op.background_brightness = 1e-3, 1.0
    call = lib.nerf_octree_backward_rays
    assert call(None, C.byref(op), C.byref(args())) == -1 and "NULL tree" in err()
    assert call(fake, C.byref(op), None) == -1 and "nerf_octree_backward_args is NULL" in err()
    assert call(fake, None, C.byref(args())) == -1 and "nerf_octree_render_options is NULL" in err()
    a = args()
    a.struct_size -= 8
    assert call(fake, C.byref(op), C.byref(a)) == -1 and "struct_size" in err()
    assert call(fake, C.byref(op), C.byref(args(n_rays=(1 << 26) + 1))) == -1 and "n_rays" in err()
    assert call(fake, C.byref(op), C.byref(args(n_rays=-1))) == -1 and "n_rays = -1" in err()
    assert call(fake, C.byref(op), C.byref(args(rgb_gt=ptr))) == -1 and "exactly one" in err()
    assert call(fake, C.byref(op), C.byref(args(grad_rgb=None))) == -1 and "exactly one" in err()
    assert call(fake, C.byref(op), C.byref(args(grad_data=None))) == -1 and "grad_data is NULL" in err()
    assert call(fake, C.byref(op), C.byref(args(loss_scale=float("nan")))) == -1 and "loss_scale" in err()
    assert lib.nerf_octree_backward_image(fake, None, C.byref(op), C.byref(args())) == -1 and "nerf_grid_camera is NULL" in err()


def test_backward_kernels_generated_code(tmp_path):
    """The backward kernels: 5 basis sizes x rays / image x plain / table-started descent x grad_rgb / fused; no inline
    assembly, float atomics as one instruction (no compare-and-swap loop), no scratch at B <= 16; VGPRs, scratch and LDS per
    kernel, printed (profiles/octree_train.md quotes them)."""
    text, asm, build = compile_kernels_to_asm(tmp_path, "octree_grad_kernels.hip")
    assert "octree_grad_kernels.hip" in build.SOURCES
    assert not re.search(r"\basm\b|__asm", text)
    for fn in ("octree_descend", "octree_setup", "octree_sh_basis", "unit_cube", "octree_act", "tile_pixel", "camera_ray"):
        assert re.search(r"\b%s\b" % fn, text) and not re.search(r"\b(void|float|int64_t)\s+%s\b" % fn, text), fn      # used, not copied
    kernels = re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M)
    assert len(kernels) == 40 and all("octree_backward" in k for k in kernels)
    scratch = dict(zip(kernels, (int(v) for v in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm))))
    vgprs = dict(zip(kernels, (int(v) for v in re.findall(r"\.vgpr_count:\s*(\d+)", asm))))
    lds = dict(zip(kernels, (int(v) for v in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", asm))))
    for k in kernels:
        print(k, "vgprs", vgprs[k], "scratch", scratch[k], "lds", lds[k])
    assert "global_atomic_add_f32" in asm and "cmpswap" not in asm
    small = [k for k in kernels if "ILi25E" not in k]
    assert len(small) == 32 and all(scratch[k] == 0 for k in small)
    assert max(vgprs.values()) <= 128      # at least 4 waves per SIMD
