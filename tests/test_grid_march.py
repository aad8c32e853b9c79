"""Sparse voxel grid: every kernel that walks a ray walks it in grid_march (csrc/grid_device.h), so all of them visit the same
samples. Here the five forwards that march - render, expected depth, taped render, taped depth, fused render + backward -
are run on one hand-made grid and one set of rays, and what they share has to be the same tensor, bit for bit: no tolerance
appears anywhere in this file. Needs a real MI355X: run with ``pytest -m gpu``."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RESO = 24
N_RAYS = 67      # 2, 4 or 16 rays per wavefront at basis_dim 9, 4, 1: the last wavefront holds a partial set of groups


@pytest.fixture(scope="module")
def N():
    import nerf_projects_amd as pkg
    return pkg


def hand_made_grid(basis_dim):
    """24^3 nodes around the origin (node i at (i - 11.5) / 12): a kept ball of radius 8 nodes, dense enough that a ray
    through its middle stops at stop_thresh, and a kept slab two nodes thick on the upper x face, thin enough to see through.
    Rows in random order; empty links are -1 or below."""
    rng = np.random.default_rng(24 + basis_dim)
    i, j, k = np.meshgrid(*(np.arange(RESO, dtype=np.float64),) * 3, indexing="ij")
    r = np.sqrt((i - 11.5) ** 2 + (j - 11.5) ** 2 + (k - 11.5) ** 2)
    ball = r <= 8.0
    slab = np.zeros_like(ball)
    slab[RESO - 2:, 4:20, 4:20] = True
    kept = ball | slab
    n = int(kept.sum())
    links = np.where(rng.uniform(size=kept.shape) < 0.5, -1, -3).astype(np.int32)
    rows = rng.permutation(n).astype(np.int32)
    links[kept] = rows
    density = np.zeros((n, 1), np.float32)
    density[links[ball], 0] = (60.0 * (1.0 - r[ball] / 9.0)).astype(np.float32)      # 60 in the middle, 6.7 at the rim
    density[links[slab & ~ball], 0] = 2.0
    sh = (0.5 * rng.normal(size=(n, 3 * basis_dim))).astype(np.float32)
    return links, density, sh


def hand_made_rays():
    """67 rays, directions not unit: 30 through the ball (9 of them along +x towards it, through the slab), 12 grazing it,
    8 missing the box, 14 starting inside it, one zero direction, one NaN origin, one infinite origin."""
    rng = np.random.default_rng(67)

    def unit(v):
        return v / np.linalg.norm(v, axis=-1, keepdims=True)

    o, d = [], []
    # through the ball: from a sphere of radius 2.5 towards a point within 0.2 of the centre
    src = 2.5 * unit(rng.normal(size=(30, 3)))
    src[:9] = [2.5, 0.0, 0.0] + 0.3 * rng.uniform(-1, 1, (9, 3))
    o.append(src)
    d.append(rng.uniform(-0.2, 0.2, (30, 3)) - src)
    # grazing: past the centre at 0.6 .. 0.72 (the ball's rim is at 8 / 12)
    src = 2.5 * unit(rng.normal(size=(12, 3)))
    side = unit(np.cross(src, rng.normal(size=(12, 3))))
    o.append(src)
    d.append(side * rng.uniform(0.6, 0.72, (12, 1)) - src)
    # missing the box: pointing away from it
    src = 2.5 * unit(rng.normal(size=(8, 3)))
    o.append(src)
    d.append(src + 0.3 * rng.normal(size=(8, 3)))
    # starting inside the box (most of them inside the ball)
    o.append(rng.uniform(-0.9, 0.9, (14, 3)))
    d.append(rng.normal(size=(14, 3)))
    o, d = np.concatenate(o), np.concatenate(d)
    d *= rng.uniform(0.25, 4.0, (len(d), 1))
    o = np.concatenate([o, [[0.1, 0.2, 2.5], [np.nan, 0.0, 2.5], [np.inf, 0.0, 0.0]]])
    d = np.concatenate([d, [[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [-1.0, 0.0, 0.0]]])
    assert o.shape == (N_RAYS, 3) and d.shape == (N_RAYS, 3)
    return o.astype(np.float32), d.astype(np.float32)


def march_everything(N, grid, rays, gt):
    """what every marching forward returns for ``rays`` on ``grid`` as it is (with or without skip data)"""
    out = {}
    out["rgb"], out["logt"] = grid.volume_render(rays, return_log_transmit=True)
    out["depth"], out["logt_depth"] = grid.volume_render_depth(rays, return_log_transmit=True)
    module = N.GridModule(grid)
    out["rgb_taped"], out["logt_taped"] = module.volume_render(rays, return_log_transmit=True)
    out["depth_taped"], out["logt_depth_taped"] = module.volume_render_depth(rays, return_log_transmit=True)
    assert out["rgb_taped"].requires_grad and out["depth_taped"].requires_grad      # the taped kernels ran, not the plain ones
    out["rgb_fused"], out["logt_fused"] = N.GridTrainer(grid).forward_backward(rays, gt, return_log_transmit=True)
    counters = torch.zeros(2, device="cuda", dtype=torch.int64)
    out["rgb_counted"] = grid._render(None, rays, False, False, counters)
    out["visited"], out["shaded"] = counters.cpu().tolist()
    return {key: v.detach() if torch.is_tensor(v) else v for key, v in out.items()}


def assert_one_lattice(out):
    for key in ("logt_depth", "logt_taped", "logt_depth_taped", "logt_fused"):
        assert torch.equal(out[key], out["logt"]), key
    for key in ("rgb_taped", "rgb_fused", "rgb_counted"):
        assert torch.equal(out[key], out["rgb"]), key
    assert torch.equal(out["depth_taped"], out["depth"])


@pytest.mark.parametrize("basis_dim", (1, 4, 9))
def test_every_marching_forward_walks_the_same_samples(N, basis_dim):
    links, density, sh = hand_made_grid(basis_dim)
    grid = N.SparseGrid.from_tensors(torch.from_numpy(links).cuda(), torch.from_numpy(density).cuda(),
                                     torch.from_numpy(sh).cuda(), [1.0, 1.0, 1.0], [0.0, 0.0, 0.0])
    o, d = hand_made_rays()
    rays = N.Rays(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda())
    gt = torch.from_numpy(np.random.default_rng(3).uniform(0, 1, (N_RAYS, 3)).astype(np.float32)).cuda()

    assert not grid.accelerated
    plain = march_everything(N, grid, rays, gt)
    assert_one_lattice(plain)
    grid.accelerate()
    assert grid.accelerated
    accel = march_everything(N, grid, rays, gt)
    assert_one_lattice(accel)

    # the rays are what the docstrings say: some stop, some end with light left, the misses and the degenerate ones see nothing
    logt = plain["logt"].cpu().numpy()
    print(f"basis_dim {basis_dim}: stopped {(logt == -1e3).sum()}, partial {((logt < 0) & (logt > -1e3)).sum()}, "
          f"untouched {(logt == 0).sum()}; visited {plain['visited']} -> {accel['visited']}, shaded {plain['shaded']}")
    assert (logt[:30] == -1e3).sum() >= 15 and ((logt[30:42] < 0) & (logt[30:42] > -1e3)).sum() >= 6
    assert (logt[42:50] == 0).all() and (logt[64:] == 0).all() and (logt[50:64] < 0).sum() >= 8
    assert np.isfinite(plain["rgb"].cpu().numpy()).all() and np.isfinite(plain["depth"].cpu().numpy()).all()

    # skip data changes which samples load links, never which are shaded or what they give
    for key in ("rgb", "logt", "depth"):
        assert torch.equal(accel[key], plain[key]), key
    assert accel["shaded"] == plain["shaded"] > 0
    assert accel["visited"] < plain["visited"]
