"""The folded stream's index tables (nerf-projects_amd/csrc/pack_weights.cpp, pack_weights_folded), on the CPU.

nerf_load_weights packs a network whose tensors hold their own flat index and whose fold - W_vf [W/2, W], b_vf [W/2] - holds
the indices behind the last parameter: the packed floats are the tables through which the device gathers the folded stream
out of parameters + tail. Here the same packer (g++, AddressSanitizer and UBSan, tests/sanitize/pack_fold_driver.cpp) makes
the tables, a numpy parameter buffer with a numpy-made fold behind it is gathered through them, and W_vf[row, col] is looked
for at the fragment positions fill_group defines. In the manner of tests/test_pack_sanitized.py."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nerf-projects_amd", "csrc")
CHUNK, TILE = 8192, 32


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = tmp_path_factory.mktemp("san") / "pack_fold_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "include"),
           "-I", CSRC, os.path.join(ROOT, "tests", "sanitize", "pack_fold_driver.cpp"), os.path.join(CSRC, "pack_weights.cpp"),
           "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out)


def hidden_col(tile, t, h):
    return 32 * tile + (t & 3) + 8 * (t >> 2) + 4 * h


def pe_col_dir(t, h):
    if t < 6:
        return 3 + 6 * (t // 3 + 2 * h) + 3 * h + t % 3
    if t < 12:
        return 3 + 6 * ((t - 6) // 3 + 2 * (1 - h)) + 3 * h + t % 3
    if t == 12:
        return 2 if h else 0
    if t == 13:
        return -1 if h else 1
    return -1


def group(at, ot, t4, col):
    """fill_group: lane = (row lane & 31, half h), four consecutive k-steps 4 t4 .. 4 t4 + 3."""
    g = np.zeros((64, 4))
    for lane in range(64):
        row, h = 32 * ot + (lane & 31), lane >> 5
        for j in range(4):
            g[lane, j] = at(row, col(4 * t4 + j, h))
    return g.reshape(-1)


@pytest.mark.parametrize("D,W,skips", [(8, 256, (4,)), (2, 100, ()), (3, 128, (0,))])
def test_folded_tables_gather_the_fold(driver, tmp_path, D, W, skips):
    out = tmp_path / "fold.bin"
    r = subprocess.run([driver, str(D), str(W), "63", "27", str(len(skips)), *map(str, skips), str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    raw = np.fromfile(out, dtype=np.float32)
    nc, nbt, fnc, fnbt, n_params, n_ids = np.fromfile(out, dtype=np.int32, count=6)
    body = raw[6:]
    sizes = [nc * CHUNK, nbt * TILE, fnc * CHUNK, fnbt * TILE]
    stream, bias, fstream, fbias = np.split(body[:sum(sizes)], np.cumsum(sizes)[:-1])
    ids = np.fromfile(out, dtype=np.int32)[6 + sum(sizes):]
    assert len(ids) == n_ids == fnc and fnc == nc - 8 and fnbt == nbt
    assert list(ids[-6:]) == [D + 1] * 4 + [D + 2, D + 1]
    n_trunk = nc - 14
    assert np.array_equal(fstream[:n_trunk * CHUNK], stream[:n_trunk * CHUNK])       # the trunk as in the plain stream
    assert np.array_equal(ids[:n_trunk], np.repeat(np.arange(D), [(2 if (i == 0 or (i - 1) in skips) else 0) + (8 if i else 0)
                                                                  for i in range(D)]))
    nv, n_dir = W // 2, 27
    tail = nv * W + nv
    tables = [(t.astype(np.int64) - 1) for t in (fstream, fbias)]
    assert all(t.max() < n_params + tail and t.min() >= -1 for t in tables)

    # parameters and a fold made here, gathered through the tables
    rng = np.random.default_rng(3)
    params = rng.standard_normal(n_params).astype(np.float32)
    trunk_in = [63 if i == 0 else (W + 63 if (i - 1) in skips else W) for i in range(D)]
    off = sum(W * n + W for n in trunk_in)
    wv = params[off:off + nv * (W + n_dir)].reshape(nv, W + n_dir)
    bv = params[off + nv * (W + n_dir):off + nv * (W + n_dir) + nv]
    off += nv * (W + n_dir) + nv
    wf, bf = params[off:off + W * W].reshape(W, W), params[off + W * W:off + W * W + W]
    off += W * W + W
    alpha = params[off:off + W]
    w_vf = (wv[:, :W].astype(np.float64) @ wf.astype(np.float64)).astype(np.float32)
    b_vf = (wv[:, :W].astype(np.float64) @ bf.astype(np.float64) + bv).astype(np.float32)
    buf = np.concatenate([params, w_vf.reshape(-1), b_vf])
    got_s, got_b = (np.where(t >= 0, buf[np.maximum(t, 0)], np.float32(0)) for t in tables)

    def hid(kt):
        return lambda t, h: hidden_col(kt, t, h) if hidden_col(kt, t, h) < W else -1

    at_vf = lambda r, c: w_vf[r, c] if (r < nv and 0 <= c) else 0.0
    for kp in range(4):          # two k-tiles per chunk: group = (ktl 4 + ot) 4 + t4
        want = np.concatenate([group(at_vf, ot, t4, hid(2 * kp + ktl)) for ktl in range(2) for ot in range(4) for t4 in range(4)])
        assert np.array_equal(got_s[(n_trunk + kp) * CHUNK:(n_trunk + kp + 1) * CHUNK], want.astype(np.float32)), kp
    at_alpha = lambda r, c: alpha[c] if (r == 0 and 0 <= c) else 0.0
    want = np.concatenate([group(at_alpha, 0, t4, hid(kt)) for kt in range(8) for t4 in range(4)])
    assert np.array_equal(got_s[(n_trunk + 4) * CHUNK:(n_trunk + 5) * CHUNK], want.astype(np.float32))
    at_dir = lambda r, c: wv[r, W + c] if (r < nv and 0 <= c < n_dir) else 0.0
    want = np.concatenate([group(at_dir, ot, t4, pe_col_dir) for ot in range(4) for t4 in range(4)])
    last = got_s[(n_trunk + 5) * CHUNK:]
    assert np.array_equal(last[:len(want)], want.astype(np.float32)) and not last[len(want):].any()
    # the bias block: b_vf in the view layer's four tiles (8 D + 9 ..), every other tile as in the plain block
    plain_b = np.where(bias > 0, params[np.maximum(bias.astype(np.int64) - 1, 0)], np.float32(0))
    v0, v1 = (8 * D + 9) * TILE, (8 * D + 13) * TILE
    assert np.array_equal(got_b[:v0], plain_b[:v0]) and np.array_equal(got_b[v1:], plain_b[v1:])
    want = [b_vf[hidden_col(ot, r, h)] if hidden_col(ot, r, h) < nv else 0.0 for ot in range(4) for h in range(2) for r in range(16)]
    assert np.array_equal(got_b[v0:v1], np.asarray(want, dtype=np.float32))
