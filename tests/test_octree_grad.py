"""PlenOctree's backward on the GPU (include/nerf_mi355x.h, "PlenOctree: backward") against tests/octree_grad_oracle.py, whose
fp64 backward tests/test_octree_grad_cpu.py pins to central differences. The bar, separately for the coefficient columns and
the sigma column, is ``max(3 d_ref, 1e-5 max|fp64 gradient|)``: ``d_ref`` is the oracle's own fp32-to-fp64 distance, the
floor is the colour tests' 1e-5 on values of order 1 scaled to the tensor (float atomics arrive in any order).
Needs a real MI355X: run with ``pytest -m gpu``."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import octree_grad_oracle as G
import octree_oracle as O

pytestmark = pytest.mark.gpu

# (activation, step_size, fast, background_brightness): tests/test_octree.py's SETTINGS
SETTINGS = [("relu_half", 1e-3, False, 1.0), ("relu_half", 1e-5, False, 0.0), ("sigmoid", 1e-3, True, 1.0),
            ("sigmoid", 1e-5, False, 1.0), ("relu_half", 1e-5, True, 0.0), ("sigmoid", 1e-3, False, 0.0)]
ALL_CASES = sorted(O.CASES) + sorted(G.DENSE)
C2W = [[0.8, 0.36, -0.48, 1.9], [0.6, -0.48, 0.64, -2.5], [0.0, -0.8, -0.6, 2.4]]      # OpenCV: z looks at the box


@pytest.fixture(scope="module")
def N():
    import nerf_projects_amd as pkg
    return pkg


def gpu(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def cpu(t):
    return t.detach().cpu().numpy()


def make_tree(N, t, act=None):
    B = (t["data"].shape[-1] - 1) // 3
    return N.N3Tree(t["child"], t["data"], t["parent_depth"], t["invradius"], t["offset"], f"SH{B}",
                    act or t["rgb_activation"], device="cuda")


def options(step, fast, bg):
    thresh = 1e-2 if fast else 0.0
    return dict(step_size=step, sigma_thresh=thresh, stop_thresh=thresh, background_brightness=bg)


@functools.lru_cache(maxsize=None)
def reference(name, act, step, fast, bg, seed=3):
    """``(g [n, 3] fp32, fp32 gradient, fp64 gradient, shaded cells)`` of a case at a setting, computed once and shared."""
    _, t, o, d = G.case(name)
    ot = O.with_activation(t, act)
    g = np.random.default_rng(seed).standard_normal((o.shape[0], 3)).astype(np.float32)
    kw = options(step, fast, bg)
    g32 = G.backward(ot, o, d, g=g, rad=np.float32, **kw)[1]
    g64 = G.backward(ot, o, d, g=g, rad=np.float64, **kw)[1]
    return g, g32, g64, G.shaded_cells(ot, o, d, **kw)


def c_backward(N, tree, kw, o=None, d=None, cam=None, g=None, gt=None, loss_scale=0.0, grad=None):
    """The C entries, called directly: ``(grad_data, rgb, loss)``."""
    from nerf_projects_amd import _lib
    h = tree._handle()
    ctx = tree._ctx
    a = _lib.OctreeBackwardArgs()
    n = cam.width * cam.height if cam is not None else o.shape[0]
    if cam is None:
        a.origins, a.dirs, a.n_rays = o.data_ptr(), d.data_ptr(), n
    grad = torch.zeros_like(tree.data) if grad is None else grad
    rgb = torch.full((n, 3), -7.0, device="cuda")
    loss = torch.zeros(1, device="cuda")
    a.grad_rgb = 0 if g is None else g.data_ptr()
    a.rgb_gt = 0 if gt is None else gt.data_ptr()
    a.loss_scale, a.grad_data, a.loss, a.rgb = loss_scale, grad.data_ptr(), loss.data_ptr(), rgb.data_ptr()
    a.capped, a.stream = tree._capped.data_ptr(), ctx.stream().value
    op = tree._options(kw["step_size"], kw["sigma_thresh"], kw["stop_thresh"], kw["background_brightness"], False)
    if cam is not None:
        c = cam._to_c()
        assert ctx.lib.nerf_octree_backward_image(h, C.byref(c), C.byref(op), C.byref(a)) == 0, ctx.lib.nerf_last_error()
    else:
        assert ctx.lib.nerf_octree_backward_rays(h, C.byref(op), C.byref(a)) == 0, ctx.lib.nerf_last_error()
    return grad, rgb, loss


def within(got, g32, g64, B, what):
    for (diff, bar), part in zip(G.bar(got, g32, g64, B), ("coefficients", "sigma")):
        print(f"{what} {part}: got {diff:.3e} / bar {bar:.3e}")
        assert diff <= bar, (what, part, diff, bar)


# ---- 6. the ray entry against the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", range(len(SETTINGS)))
@pytest.mark.parametrize("name", ALL_CASES)
def test_backward_rays_against_the_oracle(N, name, setting):
    act, step, fast, bg = SETTINGS[setting]
    _, t, o, d = G.case(name)
    B = (t["data"].shape[-1] - 1) // 3
    g, g32, g64, shaded = reference(name, act, step, fast, bg)
    tree = make_tree(N, t, act)
    kw = options(step, fast, bg)
    grad, rgb, _ = c_backward(N, tree, kw, gpu(o), gpu(d), g=gpu(g))
    want_rgb = tree.volume_render(N.Rays(gpu(o), gpu(d)), step_size=step, fast=fast, background_brightness=bg)
    assert torch.equal(rgb.view(torch.int32), want_rgb.view(torch.int32))      # the renderer's bits, the NaN ray included
    got = cpu(grad).reshape(-1, 3 * B + 1)
    assert np.isfinite(got).all()
    assert not got[~shaded].any()      # rows no ray shaded: exactly 0
    within(got, g32, g64, B, f"{name} {SETTINGS[setting]}")
    assert tree.capped_rays() == 0
    # the miss (-7) and the NaN ray (-1) alone add nothing
    pair = [-7, -1]
    alone, rgb2, _ = c_backward(N, tree, kw, gpu(o[pair]), gpu(d[pair]), g=gpu(g[pair]))
    assert not bool(alone.any()) and bool(torch.isnan(rgb2[1]).all()) and bool((rgb2[0] == bg).all())


# ---- 7. added to -----------------------------------------------------------------------------------------------------------------
def test_a_second_call_doubles_the_gradient(N):
    name, (act, step, fast, bg) = "r16x8", SETTINGS[2]
    _, t, o, d = G.case(name)
    g, g32, g64, _ = reference(name, act, step, fast, bg)
    tree = make_tree(N, t, act)
    kw = options(step, fast, bg)
    grad, _, _ = c_backward(N, tree, kw, gpu(o), gpu(d), g=gpu(g))
    grad, _, _ = c_backward(N, tree, kw, gpu(o), gpu(d), g=gpu(g), grad=grad)
    within(cpu(grad).reshape(g64.shape), 2 * g32, 2 * g64, 9, "twice")


# ---- 8. the image form ------------------------------------------------------------------------------------------------------------
def test_image_form_equals_ray_form(N):
    """A 37 x 29 camera: partial tiles on both axes."""
    _, t, _, _ = G.case("r16x8")
    tree = make_tree(N, t, "sigmoid")
    cam = N.Camera(torch.tensor(C2W), fx=30.0, fy=33.0, width=37, height=29)
    rays = cam.gen_rays()
    o, d = cpu(rays.origins), cpu(rays.dirs)
    g = np.random.default_rng(4).standard_normal((o.shape[0], 3)).astype(np.float32)
    for kw in (options(1e-3, True, 1.0), options(1e-5, False, 0.5)):
        gi, rgb_i, _ = c_backward(N, tree, kw, cam=cam, g=gpu(g))
        gr, rgb_r, _ = c_backward(N, tree, kw, rays.origins, rays.dirs, g=gpu(g))
        assert torch.equal(rgb_i.view(torch.int32), rgb_r.view(torch.int32))
        assert torch.equal(rgb_i, tree.volume_render_image(cam, **kw).view(-1, 3))
        ot = O.with_activation(t, "sigmoid")
        g32 = G.backward(ot, o, d, g=g, rad=np.float32, **kw)[1]
        g64 = G.backward(ot, o, d, g=g, rad=np.float64, **kw)[1]
        assert np.abs(g64).max() > 0
        within(cpu(gi).reshape(g64.shape), g32, g64, 9, "image form")
        within(cpu(gr).reshape(g64.shape), g32, g64, 9, "ray form")


# ---- 9. accelerate -----------------------------------------------------------------------------------------------------------------
def test_accelerated_backward_equals_the_plain_one(N):
    name, (act, step, fast, bg) = "r16", SETTINGS[2]
    _, t, o, d = G.case(name)
    g, g32, g64, _ = reference(name, act, step, fast, bg)
    tree = make_tree(N, t, act)
    kw = options(step, fast, bg)
    cam = N.Camera(torch.tensor(C2W), fx=22.0, fy=25.0, width=24, height=20)
    gi = torch.randn(24 * 20, 3, device="cuda", generator=torch.Generator("cuda").manual_seed(0))
    _, plain_rgb, _ = c_backward(N, tree, kw, gpu(o), gpu(d), g=gpu(g))
    plain_img, plain_img_rgb, _ = c_backward(N, tree, kw, cam=cam, g=gi)
    for levels, k in ((1, 1), (3, 3), (6, 3)):      # below, at and above max_depth (3)
        assert tree.accelerate(levels) == k
        grad, rgb, _ = c_backward(N, tree, kw, gpu(o), gpu(d), g=gpu(g))
        assert torch.equal(rgb.view(torch.int32), plain_rgb.view(torch.int32))
        within(cpu(grad).reshape(g64.shape), g32, g64, 9, f"accelerate({levels})")
        img, img_rgb, _ = c_backward(N, tree, kw, cam=cam, g=gi)
        assert torch.equal(img_rgb, plain_img_rgb)
        scale = float(plain_img.abs().max())
        assert scale > 0 and float((img - plain_img).abs().max()) <= 1e-5 * scale      # the same terms, in another order
    assert tree.accelerate(0) == 0


# ---- 10. autograd ------------------------------------------------------------------------------------------------------------------
def test_autograd_through_the_renders(N):
    name, (act, step, fast, bg) = "r8x8", SETTINGS[4]
    _, t, o, d = G.case(name)
    g, g32, g64, _ = reference(name, act, step, fast, bg)
    kw = options(step, fast, bg)
    tree = make_tree(N, t, act).requires_grad_()
    rays = N.Rays(gpu(o), gpu(d))
    plain = make_tree(N, t, act).volume_render(rays, **kw)
    out, steps = tree.volume_render(rays, return_steps=True, **kw)
    assert out.grad_fn is not None and not steps.requires_grad and torch.equal(out.view(torch.int32), plain.view(torch.int32))
    (out * gpu(g)).sum().backward()      # (the NaN ray makes the sum NaN, not the gradient: it is g for every ray)
    within(cpu(tree.data.grad).reshape(g64.shape), g32, g64, 4, "volume_render")
    with torch.no_grad():
        assert tree.volume_render(rays, **kw).grad_fn is None
    assert make_tree(N, t, act).volume_render(rays, **kw).grad_fn is None
    with pytest.raises(NotImplementedError, match="rays"):
        tree.volume_render(N.Rays(gpu(o).requires_grad_(), gpu(d)))
    # the image forms
    cam = N.Camera(torch.tensor(C2W), fx=30.0, fy=33.0, width=37, height=29)
    cr = cam.gen_rays()
    gi = np.random.default_rng(6).standard_normal((29, 37, 3)).astype(np.float32)
    ot = O.with_activation(t, act)
    i32 = G.backward(ot, cpu(cr.origins), cpu(cr.dirs), g=gi.reshape(-1, 3), rad=np.float32, **kw)[1]
    i64 = G.backward(ot, cpu(cr.origins), cpu(cr.dirs), g=gi.reshape(-1, 3), rad=np.float64, **kw)[1]
    tree.data.grad = None
    img = tree.volume_render_image(cam, **kw)
    assert img.shape == (29, 37, 3) and img.grad_fn is not None
    (img * gpu(gi)).sum().backward()
    within(cpu(tree.data.grad).reshape(i64.shape), i32, i64, 4, "volume_render_image")
    pose = torch.tensor([[0.8, -0.36, 0.48, 1.9], [0.6, 0.48, -0.64, -2.5], [0.0, 0.8, 0.6, 2.4], [0.0, 0.0, 0.0, 1.0]])      # OpenGL
    pc = N.Camera.from_nerf_pose(pose, 20, 24, 22.0).gen_rays()
    gp = np.random.default_rng(7).standard_normal((20, 24, 3)).astype(np.float32)
    p32 = G.backward(ot, cpu(pc.origins), cpu(pc.dirs), g=gp.reshape(-1, 3), rad=np.float32, **kw)[1]
    p64 = G.backward(ot, cpu(pc.origins), cpu(pc.dirs), g=gp.reshape(-1, 3), rad=np.float64, **kw)[1]
    tree.data.grad = None
    (tree.render_persp(pose, width=24, height=20, fx=22.0, **kw) * gpu(gp)).sum().backward()
    assert np.abs(p64).max() > 0
    within(cpu(tree.data.grad).reshape(p64.shape), p32, p64, 4, "render_persp")
    # optimization.py's inner loop, literally
    tree.data.grad = None
    optimizer = torch.optim.SGD(tree.parameters(), lr=1e-3)
    before = tree.data.detach().clone()
    im_gt = torch.rand(20, 24, 3, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    for _ in range(2):
        im = tree.render_persp(pose, width=24, height=20, fx=22.0, **kw)
        im = im.clamp(0.0, 1.0)
        mse = ((im - im_gt) ** 2).mean()
        optimizer.zero_grad()
        mse.backward()
        optimizer.step()
    assert bool(torch.isfinite(tree.data).all()) and not torch.equal(tree.data.detach(), before)


# ---- 11. the fused form -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,act", [("r16x8", "relu_half"), ("r8x8", "relu_half"), ("r16", "sigmoid")])
def test_mse_backward_equals_clamp_mse_autograd(N, name, act):
    _, t, o, d = G.case(name)
    B = (t["data"].shape[-1] - 1) // 3
    ot = O.with_activation(t, act)
    kw = options(1e-3, True, 1.0)
    n = o.shape[0]
    gt = np.random.default_rng(12).random((n, 3)).astype(np.float32)
    scale = 2.0 / (3 * n)
    _, g32, lsum32, _ = G.backward(ot, o, d, rgb_gt=gt, loss_scale=scale, rad=np.float32, **kw)
    rgb64, g64, lsum64, _ = G.backward(ot, o, d, rgb_gt=gt, loss_scale=scale, rad=np.float64, **kw)
    rays = N.Rays(gpu(o[:-1]), gpu(d[:-1]))      # torch's loss of the NaN ray would be NaN: the fused form's documented deviation
    # torch: clamp + MSE through the autograd render, on the rays without the NaN one, scaled to the same 3 n
    tree = make_tree(N, t, act).requires_grad_()
    im = tree.volume_render(rays, **kw).clamp(0.0, 1.0)
    mse = ((im - gpu(gt[:-1])) ** 2).sum() / (3 * n)
    mse.backward()
    within(cpu(tree.data.grad).reshape(g64.shape), g32, g64, B, "autograd clamp + mse")
    # fused, with the NaN ray
    fused = make_tree(N, t, act).requires_grad_()
    assert fused.data.grad is None
    loss = fused.mse_backward(N.Rays(gpu(o), gpu(d)), gpu(gt), **kw)
    assert loss.dim() == 0 and loss.is_cuda and fused.data.grad is not None
    within(cpu(fused.data.grad).reshape(g64.shape), g32, g64, B, "mse_backward")
    loss, mse = float(loss), float(mse.detach())
    rel = abs(loss - mse) / mse
    print(f"{name}: fused loss {loss:.8g}, torch {mse:.8g} (rel {rel:.2e}), oracle {lsum64 / (3 * n):.8g}")
    assert rel <= 1e-6 and abs(loss - lsum64 / (3 * n)) <= 1e-6 * mse
    # added to: a second call doubles it
    fused.mse_backward(N.Rays(gpu(o), gpu(d)), gpu(gt), **kw)
    within(cpu(fused.data.grad).reshape(g64.shape), 2 * g32, 2 * g64, B, "mse_backward twice")
    if act == "relu_half" and name in G.DENSE:
        # channels outside [0, 1] get no gradient, and that matters: without the mask the oracle is far outside the bar
        outside = ((rgb64 < 0) | (rgb64 > 1)).any(1)
        assert outside.sum() >= 1
        unmasked = G.backward(ot, o, d, rgb_gt=gt, loss_scale=scale, clamp_mask=False, rad=np.float64, **kw)[1]
        bars = G.bar(unmasked, g32, g64, B)
        print("without the mask:", bars)
        assert any(diff > 10 * bar for diff, bar in bars)


# ---- 12. a descent step -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["r8", "r8x8", "r16"])
def test_descent_step_on_the_gpu(N, name):
    """tests/test_octree_grad_cpu.py's step with mse_backward and a plain data.sub_: the CPU band [0.97, 1.01] widened to
    [0.95, 1.02] for the fp32 loss sums (the decrease is 1e-2 of the loss, four orders of magnitude above that noise)."""
    _, t, o, d = G.case(name)
    kw = options(1e-3, True, 1.0)
    rays = N.Rays(gpu(o), gpu(d))
    gt = gpu(np.random.default_rng(11).random((o.shape[0], 3)).astype(np.float32))
    tree = make_tree(N, t)
    L0 = float(tree.mse_backward(rays, gt, **kw))
    grad = tree.data.grad
    g2 = float((grad.double() ** 2).sum())
    lr = 1e-2 * L0 / g2
    with torch.no_grad():
        tree.data.sub_(lr * grad)
    L1 = float(tree.mse_backward(rays, gt, **kw))
    ratio = (L0 - L1) / (lr * g2)
    print(f"{name}: L0 {L0:.6g} L1 {L1:.6g} ratio {ratio:.4f}")
    assert 0.95 <= ratio <= 1.02


# ---- 13. optimize -----------------------------------------------------------------------------------------------------------------
def test_optimize_follows_the_loop(N):
    from nerf_projects_amd.octree_optimize import optimize
    _, t, _, _ = G.case("r8")
    truth = make_tree(N, t)
    poses = []
    for k in range(6):      # cameras on a circle of radius 3.2 looking at the box (OpenCV: z forward, y down)
        th = 2 * np.pi * k / 6 + 0.3
        eye = np.array([3.2 * np.cos(th), 3.2 * np.sin(th), 1.1 + 0.2 * k])
        z = -eye / np.linalg.norm(eye)
        x = np.cross(z, [0.0, 0.0, 1.0])
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        poses.append(torch.tensor(np.stack([x, y, z, eye], 1), dtype=torch.float32))
    cams = [N.Camera(p, fx=40.0, width=32, height=32) for p in poses]
    kw = dict(step_size=1e-3, fast=True)
    images = [truth.volume_render_image(c, **kw).clamp(0.0, 1.0) for c in cams]
    assert float(torch.stack(images).std()) > 0.05      # the cameras see the tree
    noisy = truth.data + 0.3 * torch.randn(truth.data.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(2))
    start = N.N3Tree(truth.child.clone(), noisy.clone(), truth.parent_depth, truth.invradius, truth.offset, "SH4", "relu_half")
    child_before = start.child.clone()
    probe = start.clone()
    L0 = float(probe.mse_backward(cams[0], images[0], **kw))
    lr = 5e-2 * L0 / float((probe.data.grad.double() ** 2).sum())
    best, hist = optimize(start, cams[:4], images[:4], cams[4:], images[4:], num_epochs=3, lr=lr, continue_on_decrease=True, **kw)
    print("optimize:", hist)
    assert len(hist["train_psnr"]) == 3 and [e for e, _ in hist["val_psnr"]] == [1, 2]
    assert hist["train_psnr"][-1] > hist["train_psnr"][0]
    assert torch.equal(start.child, child_before) and start.data.requires_grad
    assert best is None or (isinstance(best, N.N3Tree) and best.data.data_ptr() != start.data.data_ptr())
    # lr = 0: renders are bit-reproducible, so the validation PSNR is equal, not greater: no best tree, and the loop ends
    still = N.N3Tree(truth.child.clone(), noisy.clone(), truth.parent_depth, truth.invradius, truth.offset, "SH4", "relu_half")
    best, hist = optimize(still, cams[:4], images[:4], cams[4:], images[4:], num_epochs=6, lr=0.0, **kw)
    assert best is None and len(hist["val_psnr"]) == 1 and hist["val_psnr"][0] == (1, hist["initial_val_psnr"])
    assert len(hist["train_psnr"]) == 2 and torch.equal(still.data.detach(), noisy)
    best, hist = optimize(still, cams[:2], images[:2], cams[4:], images[4:], num_epochs=1, lr=1e-3, sgd=False, **kw)      # Adam runs
    assert len(hist["train_psnr"]) == 1 and bool(torch.isfinite(still.data).all())


# ---- 14. the C entries' refusals -------------------------------------------------------------------------------------------------
def test_c_entries_refuse_bad_arguments(N):
    from nerf_projects_amd import _lib
    _, t, o, d = O.case("r8")
    tree = make_tree(N, t)
    h = tree._handle()
    lib, ctx = tree._ctx.lib, tree._ctx
    err = lambda: lib.nerf_last_error().decode()      # noqa: E731
    host = np.zeros(1 << 16, np.float32)
    rays_o, rays_d = gpu(o[:16]), gpu(d[:16])
    g = torch.ones(16, 3, device="cuda")
    grad = torch.full_like(tree.data, -7.0)      # poisoned: a launch would change it
    loss = torch.full((1,), -7.0, device="cuda")

    def args(**k):
        a = _lib.OctreeBackwardArgs()
        a.origins, a.dirs, a.n_rays, a.grad_rgb = rays_o.data_ptr(), rays_d.data_ptr(), 16, g.data_ptr()
        a.grad_data, a.loss, a.loss_scale, a.stream = grad.data_ptr(), loss.data_ptr(), 1.0, ctx.stream().value
        for name, v in k.items():
            setattr(a, name, v)
        return a

    op = _lib.OctreeRenderOptions()
    op.step_size, op.background_brightness = 1e-3, 1.0
    call = lib.nerf_octree_backward_rays
    bad = lambda a: call(h, C.byref(op), C.byref(a)) == -1      # noqa: E731  (NERF_E_INVALID)
    assert bad(args(rgb_gt=g.data_ptr())) and "exactly one" in err()
    assert bad(args(grad_rgb=None)) and "exactly one" in err()
    assert bad(args(grad_data=None)) and "grad_data is NULL" in err()
    for name in ("origins", "dirs", "grad_rgb", "grad_data", "loss", "rgb", "capped"):
        assert bad(args(**{name: host.ctypes.data})) and f"{name} is not device memory" in err(), name
    assert bad(args(grad_rgb=None, rgb_gt=host.ctypes.data)) and "rgb_gt is not device memory" in err()
    assert bad(args(n_rays=(1 << 26) + 1)) and "n_rays" in err()
    short = args()
    short.struct_size -= 8
    assert bad(short) and "struct_size" in err()
    assert call(None, C.byref(op), C.byref(args())) == -1 and "NULL tree" in err()
    cam = N.Camera(torch.eye(4)[:3], fx=10.0, width=4, height=4)._to_c()
    assert lib.nerf_octree_backward_image(h, C.byref(cam), C.byref(op), C.byref(args(grad_data=host.ctypes.data))) == -1
    assert lib.nerf_octree_backward_image(h, None, C.byref(op), C.byref(args())) == -1
    torch.cuda.synchronize()
    assert bool((grad == -7.0).all()) and float(loss) == -7.0      # nothing was launched
    assert call(h, C.byref(op), C.byref(args())) == 0      # and the good call goes through
    torch.cuda.synchronize()
    assert not bool((grad == -7.0).all())
