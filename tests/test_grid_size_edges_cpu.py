"""Sparse voxel grid at the size limits of the C ABI, the part that needs no GPU: the inputs tests/test_grid_size_edges.py feeds
the kernels are what its docstrings say, judged by the numpy oracle alone, so that they cannot silently go trivial - the rays on
the lattices of 2 and 1024 nodes stop, end with light left and miss; the skip distances reach their cap; skipping saves links
and changes nothing; the sample points sit outside the box, on its faces and on nodes; and a table laid out for the large
tests has its first linked entry past 2^31."""
import numpy as np
import pytest

import grid_oracle as GO
import grid_size_edges_lib as L


@pytest.mark.parametrize("reso,basis_dim", L.EDGE_LATTICES)
def test_the_rays_on_the_edge_lattices_do_what_they_are_meant_to(reso, basis_dim):
    g = L.edge_grid(reso, basis_dim)
    o, d = L.edge_rays(g)
    assert g["links"].shape == tuple(reso) and g["sh_data"].shape[1] == 3 * basis_dim and o.shape == (L.EDGE_RAYS, 3)
    assert (g["links"] == -1).any() and (g["links"] == -3).any() if max(reso) > 2 else (g["links"] < 0).any()
    assert np.abs(np.linalg.norm(d, axis=-1) - 1).max() > 0.5      # directions are not unit
    c = L.ray_classes(g, o, d)
    print(reso, c)
    assert c["same"] and c["shaded"] == c["shaded_skip"] > 0
    assert c["stopped"] + c["partial"] + c["untouched"] == L.EDGE_RAYS
    if max(reso) == 2:
        assert c["stopped"] >= 20 and c["partial"] >= 10
        assert c["max_skip"] == 0 or c["visited_skip"] <= c["visited"]
        return
    assert c["stopped"] >= 10 and c["partial"] >= 30 and c["untouched"] >= 10
    assert c["max_skip"] == GO.SKIP_CAP == 32
    assert c["visited_skip"] <= 0.6 * c["visited"]
    # the bands: along the long axis both kept and empty stretches of 80 nodes
    axis = int(np.argmax(reso))
    any_kept = (g["links"] >= 0).any(tuple(a for a in range(3) if a != axis))
    assert any_kept[:L.BAND].mean() > 0.9 and not any_kept[L.BAND:2 * L.BAND].any()
    assert np.allclose(g["radius"] * max(reso), reso)      # cubic cells


@pytest.mark.parametrize("reso,basis_dim", L.EDGE_LATTICES)
def test_the_sample_points_cover_outside_faces_and_nodes(reso, basis_dim):
    g = L.edge_grid(reso, basis_dim)
    p = L.edge_points(g).astype(np.float64)
    size = np.array(reso, np.float64)
    outside = ((p < -0.5) | (p > size - 0.5)).any(-1)
    on_face = ((p == -0.5) | (p == size - 0.5)).any(-1)
    on_node = (p == np.floor(p)).all(-1) & (p >= 0).all(-1) & (p <= size - 1).all(-1)
    assert outside.sum() >= 64 and on_face.sum() >= 48 and on_node.sum() >= 48
    assert ((p == -0.5).any(-1)).sum() >= 10 and ((p == size - 0.5).any(-1)).sum() >= 10      # lower and upper faces
    corners = {tuple(c) for c in p[on_node].tolist()} & {(x, y, z) for x in (0.0, size[0] - 1) for y in (0.0, size[1] - 1)
                                                          for z in (0.0, size[2] - 1)}
    assert len(corners) == 8
    # on a node the sample is the node's row (or 0 where it is empty), bit for bit
    dens, sh = GO.sample(g, p[on_node].astype(np.float32), grid_coords=True)
    idx = p[on_node].astype(np.int64)
    lk = g["links"][idx[:, 0], idx[:, 1], idx[:, 2]]
    want = np.where(lk[:, None] >= 0, g["density_data"][np.maximum(lk, 0)], np.float32(0.0))
    assert np.array_equal(dens, want) and (lk >= 0).sum() >= 10 and (lk < 0).sum() >= 5
    # an axis of 2 nodes has the one base cell 0
    l, _ = GO._cell(p.astype(np.float32), reso)
    for a in range(3):
        if reso[a] == 2:
            assert (l[:, a] == 0).all()


def test_the_large_layout_puts_the_first_linked_entry_past_two_to_the_31():
    links, density, sh = L.hand_made_grid(9)
    n_tail = density.shape[0]
    assert n_tail == int((links >= 0).sum()) and sorted(links[links >= 0].tolist()) == list(range(n_tail))
    cap = L.large_capacity(n_tail)
    row0 = cap - n_tail
    assert row0 == 79_536_432 and row0 * 27 >= 2 ** 31 > (row0 - 1) * 27      # sh_data, grad_sh, sh_rms
    assert row0 * 32 >= 2 ** 31 and row0 >= 67_108_864                       # a packed half row is 32 halfs
    assert cap <= 2 ** 31 - 1 and int(links.max()) + row0 == cap - 1         # every shifted link is an int32 below capacity
    # the oracle sees on the small grid what test_grid_march.py asks of it: rays that stop, rays that end with light left
    o, d = L.hand_made_rays()
    c = L.ray_classes(L.hand_made_dict(9), o, d)
    assert c["same"] and c["stopped"] >= 15 and c["partial"] >= 10 and c["untouched"] >= 11 and c["visited_skip"] < c["visited"]
