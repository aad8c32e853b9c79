"""The sparse voxel grid's regularisers as differentiable values on the GPU (include/nerf_mi355x.h, "Sparse voxel grid:
regularisers as values"): GridModule.tv / tv_color / sparsity_loss against the fp64 statements and the restatements of
tests/grid_regularisers_oracle.py (the cases are built once in tests/test_grid_regularisers_cpu.py), against the fused
training kernel's sparsity gradient, the module's contract, and an Adam loop on the full objective.
Needs a real MI355X: run with ``pytest -m gpu``."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import grid_regularisers_oracle as RO
from test_grid import cpu, gpu, make_grid, random_grid, set_opt
from test_grid_regularisers_cpu import ROW0, SPARSITY_BATCHES, SPARSITY_OPT, TV_CASES, sparsity_case, tv_case, tv_lattice
from test_grid_train import through_rays

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def N():
    import nerf_projects_amd as pkg
    return pkg


def tv_call(m, target, d0, d1, cells):
    return m.tv(cells=cells) if target == "density" else m.tv_color(d0, d1, cells=cells)


def grads(m):
    return tuple(None if p.grad is None else cpu(p.grad).astype(np.float64) for p in (m.density_data, m.sh_data))


# ---- 1. total variation: value, bits, gradient, cotangent, accumulation -------------------------------------------------
@pytest.mark.parametrize("listed", [False, True])
@pytest.mark.parametrize("reso,basis_dim,target,d0,d1", TV_CASES)
def test_tv_value_and_gradient(N, reso, basis_dim, target, d0, d1, listed):
    """Value: |got - want64| <= 1e-6 want64 (every term is positive and formed by at most eight fp32 roundings of 2^-24, the
    fp64 sum adds nothing visible, the final rounding 6e-8); three calls return identical bits. Gradient: 1e-5 of the largest
    entry of the fp64 gradient, against fp64 autograd and against the restatement; the other table gets none; a cotangent of 3
    on the device gives three times the gradient; two backward calls accumulate."""
    g, plateau, cells, v32, v64, g64, g32 = tv_case(reso, basis_dim, target, d0, d1, listed)
    m = N.GridModule(make_grid(N, g))
    dcells = None if cells is None else gpu(cells if reso != (6, 6, 6) else cells.astype(np.int32))      # both index types
    vals = [tv_call(m, target, d0, d1, dcells) for _ in range(3)]
    got = float(vals[0].detach())
    print(f"tv {reso} B={basis_dim} {target}[{d0}:{d1}] {'list' if listed else 'dense'}: got {got:.9g} want64 {v64:.9g} "
          f"off by {abs(got - v64) / v64:.2e} (bar 1e-6); restatement {float(v32):.9g}")
    for v in vals:
        assert v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda and v.requires_grad
        assert cpu(v).tobytes() == cpu(vals[0]).tobytes()
    assert abs(got - v64) <= 1e-6 * v64
    which = 0 if target == "density" else 1
    big = float(np.abs(g64).max())
    vals[0].backward()
    once = grads(m)
    e64, e32 = np.abs(once[which] - g64).max(), np.abs(once[which] - g32).max()
    print(f"    gradient vs fp64 autograd {e64 / big:.2e}, vs restatement {e32 / big:.2e} of the largest entry (bar 1e-5)")
    assert once[1 - which] is None      # the other table gets no gradient
    assert np.isfinite(once[which]).all() and e64 <= 1e-5 * big and e32 <= 1e-5 * big
    if not listed:
        assert not once[which][plateau].any()      # the plateau: exactly 0
    vals[1].backward()      # a second backward accumulates into .grad
    assert np.abs(grads(m)[which] - 2.0 * g64).max() <= 2e-5 * big
    for p in m.parameters():
        p.grad = None
    (3.0 * vals[2]).backward()      # the cotangent is a device tensor: nothing is read back
    assert np.abs(grads(m)[which] - 3.0 * g64).max() <= 3e-5 * big


def test_tv_of_nothing_is_zero_and_has_no_gradient(N):
    g, _ = tv_lattice((9, 8, 7), 9)
    m = N.GridModule(make_grid(N, g))
    empty = torch.zeros(0, dtype=torch.int64, device="cuda")
    for v in (m.tv(cells=empty), m.tv_color(cells=empty), m.tv_color(5, 5), m.tv_color(-1, -1), m.tv_color(27, None)):
        assert v.dim() == 0 and float(v) == 0.0
        v.backward()
    assert m.density_data.grad is None and m.sh_data.grad is None
    # negative dims wrap as in svox2
    assert cpu(m.tv_color(-24, -16)).tobytes() == cpu(m.tv_color(3, 11)).tobytes()
    with pytest.raises(ValueError, match="columns"):
        m.tv_color(5, 3)
    with pytest.raises(ValueError, match="columns"):
        m.tv_color(0, 28)
    with pytest.raises(NotImplementedError, match="logalpha"):
        m.tv(logalpha=True)
    assert cpu(m.tv(ndc_coeffs=(0.5, 0.5))).tobytes() == cpu(m.tv()).tobytes()      # accepted, no effect
    # a list holding only the cell whose link is row 0: nothing with the edge rule, something without
    row0 = gpu(np.array([np.ravel_multi_index(ROW0, (9, 8, 7))], np.int64))
    assert float(m.tv_color(cells=row0)) == 0.0 and float(m.tv(cells=row0)) > 0.0


# ---- 2. the sparsity term ------------------------------------------------------------------------------------------------
def sparsity_module(N, basis_dim):
    g = sparsity_case(basis_dim)[0]
    grid = make_grid(N, g)
    set_opt(grid, 1.0, SPARSITY_OPT["step_size"], SPARSITY_OPT["near_clip"], SPARSITY_OPT["sigma_thresh"], SPARSITY_OPT["stop_thresh"])
    return grid, N.GridModule(grid)


@pytest.mark.parametrize("basis_dim", [9, 1])
def test_sparsity_value_and_gradient(N, basis_dim):
    """Value per ray: |got - want64| <= (n_r + 16) 2^-24 want64 (one rounding per accumulation plus the few of a term); misses
    and hostile rays exactly 0; plain and accelerated bit-identical; every batch size a prefix of the same rays. Gradient:
    1e-5 of the largest entry against fp64 autograd over the same sample set, with a random cotangent per ray."""
    g, o, d, s32, s64, count, g64, g32, cot, _ = sparsity_case(basis_dim)
    grid, m = sparsity_module(N, basis_dim)
    rays = N.Rays(gpu(o), gpu(d))
    plain = m.sparsity_loss(rays)
    assert plain.shape == (257,) and plain.dtype == torch.float32 and plain.requires_grad
    got = cpu(plain).astype(np.float64)
    off = np.abs(got - s64)
    bound = (count + 16) * 2.0 ** -24 * s64
    print(f"sparsity B={basis_dim}: worst ray off by {np.max(off / np.maximum(bound, 1e-300)):.2f} of its bound; "
          f"{int((count > 0).sum())} rays shaded, {int((cpu(plain) != s32).sum())} differ from the fp32 restatement")
    assert (off <= bound).all()
    assert not got[-8:].any() and not got[count == 0].any()
    (plain * gpu(cot)).sum().backward()
    gd = grads(m)
    big = float(np.abs(g64).max())
    e64, e32 = np.abs(gd[0] - g64).max(), np.abs(gd[0] - g32).max()
    print(f"    gradient vs fp64 autograd {e64 / big:.2e}, vs restatement {e32 / big:.2e} of the largest entry (bar 1e-5)")
    assert gd[1] is None and np.isfinite(gd[0]).all() and e64 <= 1e-5 * big and e32 <= 1e-5 * big
    grid.accelerate()
    fast = m.sparsity_loss(rays)
    assert grid.accelerated and torch.equal(fast, plain)
    m.density_data.grad = None
    (fast * gpu(cot)).sum().backward()
    assert np.abs(grads(m)[0] - g64).max() <= 1e-5 * big
    for n in SPARSITY_BATCHES:
        part = m.sparsity_loss(N.Rays(gpu(o[:n]), gpu(d[:n])))
        assert part.shape == (n,) and torch.equal(part, plain[:n]), n
    assert m.sparsity_loss(N.Rays(gpu(o[:0]), gpu(d[:0]))).shape == (0,)


@pytest.mark.parametrize("basis_dim", [9, 1])
def test_sparsity_gradient_is_the_fused_kernels(N, basis_dim):
    """With rgb_gt the grid's own render the colour gradient of the fused step vanishes identically: its grad_density is then
    lambda times the gradient of sparsity_loss(rays).sum(), within 1e-5 of the largest entry, and grad_sh exactly 0."""
    g, o, d = sparsity_case(basis_dim)[:3]
    grid, m = sparsity_module(N, basis_dim)
    grid.accelerate()
    rays = N.Rays(gpu(o), gpu(d))
    lam = 0.37
    trainer = N.GridTrainer(grid)
    trainer.volume_render_fused(rays, grid.volume_render(rays), sparsity_loss=lam)
    m.sparsity_loss(rays).sum().backward()
    want = lam * grads(m)[0]
    got = cpu(trainer.grad_density).astype(np.float64)
    big = float(np.abs(want).max())
    print(f"fused vs sparsity_loss B={basis_dim}: {np.abs(got - want).max() / big:.2e} of the largest entry (bar 1e-5)")
    assert big > 0 and np.abs(got - want).max() <= 1e-5 * big
    assert not cpu(trainer.grad_sh).any()


# ---- 3. the module's contract -------------------------------------------------------------------------------------------
def test_module_contract(N):
    g, o, d = sparsity_case(9)[:3]
    grid, m = sparsity_module(N, 9)
    grid.accelerate()
    rays = N.Rays(gpu(o[:65]), gpu(d[:65]))
    # frozen parameters: plain results, nothing to run backward through, .grad stays None
    m.density_data.requires_grad_(False)
    assert not m.tv().requires_grad and not m.sparsity_loss(rays).requires_grad and m.tv_color().requires_grad
    (m.tv() + m.tv_color() + m.sparsity_loss(rays).sum()).backward()
    assert m.density_data.grad is None and m.sh_data.grad is not None
    m.density_data.requires_grad_(True)
    m.sh_data.requires_grad_(False)
    m.sh_data.grad = None
    assert not m.tv_color().requires_grad
    (m.tv() + m.tv_color()).backward()
    assert m.sh_data.grad is None and m.density_data.grad is not None
    m.sh_data.requires_grad_(True)
    with torch.no_grad():
        assert not m.tv().requires_grad and not m.sparsity_loss(rays).requires_grad
    # an in-place step between forward and backward
    for make in (m.tv, m.tv_color, lambda: m.sparsity_loss(rays).sum()):
        v = make()
        with torch.no_grad():
            m.density_data.add_(0.0)
            m.sh_data.add_(0.0)
        with pytest.raises(RuntimeError, match="modified by an inplace operation"):
            v.backward()
    # refusals in the existing words
    with pytest.raises(RuntimeError, match="CPU"):
        m.sparsity_loss(N.Rays(torch.zeros(4, 3), torch.ones(4, 3)))
    with pytest.raises(RuntimeError, match="CPU"):
        m.tv(cells=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(TypeError, match="int32 or int64"):
        m.tv(cells=torch.zeros(4, device="cuda"))
    with pytest.raises(NotImplementedError, match="requires a gradient"):
        m.sparsity_loss(N.Rays(gpu(o[:4]).requires_grad_(True), gpu(d[:4])))
    with pytest.raises(NotImplementedError, match="requires a gradient"):
        m.sparsity_loss(N.Rays(gpu(o[:4]), gpu(d[:4]).requires_grad_(True)))
    assert grid.accelerated
    # HalfGrid / BackgroundGrid
    half = grid.to_half()
    from nerf_projects_amd import _lib
    a = _lib.GridTvValueArgs()
    a.target, a.end_dim, a.ignore_edge, a.value = _lib.NERF_GRID_TV_SH, 27, 1, 0x1000
    assert grid.ctx.lib.nerf_grid_tv_value(half._handle(), C.byref(a)) == -1      # the SH target on a half-precision handle
    mh = N.GridModule(grid)
    mh.grid = half
    for call in (mh.tv, mh.tv_color, lambda: mh.sparsity_loss(rays)):
        with pytest.raises(TypeError, match=r"to_float\(\)"):
            call()
    mh.grid = types.SimpleNamespace(is_half=False, use_background=True)
    for call in (mh.tv, mh.tv_color, lambda: mh.sparsity_loss(rays)):
        with pytest.raises(NotImplementedError, match=r"foreground\(\)"):
            call()
    # replaced tables: refused until rebind(), then the methods run on the new tables
    before = float(m.tv())
    grid.density_data = (grid.density_data * 2.0).contiguous()
    with pytest.raises(RuntimeError, match="rebind"):
        m.tv()
    with pytest.raises(RuntimeError, match="rebind"):
        m.sparsity_loss(rays)
    m.rebind()
    g2 = dict(g, density_data=cpu(grid.density_data))
    want = RO.tv_autograd64(g2, "density")[0]
    assert abs(float(m.tv()) - want) <= 1e-6 * want and abs(want - 2.0 * before) <= 1e-3 * want
    s = m.sparsity_loss(rays)
    s.sum().backward()
    assert m.density_data.grad is not None and float(s.sum()) > 0


# ---- 4. a training loop on the full objective ---------------------------------------------------------------------------
def test_adam_loop_on_the_full_objective(N):
    """30 Adam steps on a (16, 16, 16) grid: MSE, TV on both tables (the colour TV on random cells), sparsity and the beta
    term written from log_transmit. The loss decreases and every table stays finite."""
    rng = np.random.default_rng(77)
    g = random_grid(rng, (16, 16, 16), 9, keep=0.5)
    g["density_data"] = np.abs(g["density_data"]) * 0.2
    grid = make_grid(N, g)
    grid.accelerate()
    m = N.GridModule(grid)
    o, d = through_rays(rng, g, 512)
    rays = N.Rays(gpu(o), gpu(d))
    target = gpu(rng.uniform(0.2, 0.8, (512, 3)).astype(np.float32))
    adam = torch.optim.Adam([{"params": [m.density_data], "lr": 0.2}, {"params": [m.sh_data], "lr": 1e-2}])
    gen = torch.Generator(device="cuda").manual_seed(1)
    losses = []
    for _ in range(30):
        adam.zero_grad()
        rgb, log_t = m.volume_render(rays, return_log_transmit=True)
        cells = torch.randint(0, 16 ** 3, (400,), device="cuda", generator=gen)
        beta = (log_t + torch.log(1.0 - torch.exp(log_t) + 1e-3)).mean()
        loss = (((rgb - target) ** 2).mean() + 1e-1 * m.tv() + 1e-2 * m.tv_color(cells=cells)
                + 1e-5 * m.sparsity_loss(rays).sum() + 1e-3 * beta)
        loss.backward()
        adam.step()
        losses.append(float(loss))
    print("loss", " ".join(f"{v:.4f}" for v in losses[::5]), f"-> {losses[-1]:.4f}")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    assert torch.isfinite(grid.density_data).all() and torch.isfinite(grid.sh_data).all() and grid.accelerated
