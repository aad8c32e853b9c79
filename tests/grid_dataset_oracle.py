"""numpy restatement of csrc/grid_dataset_kernels.hip (include/nerf_mi355x.h, "Sparse voxel grid: training data"): the order
``sigma`` on integers, the rays of svox2's ``gen_rays`` in fp32 with every operation rounded, the compositing and the area
windows. Every float below is an ``np.float32`` array and every numpy operation on such arrays rounds once, so the kernel's
rounded operations are restated one for one; the test files share this module (a plain module, no fixtures)."""
import numpy as np

IDENTITY, PERMUTED, RANDOM = 0, 1, 2
ROUNDS = 4
F = np.float32
U32 = np.uint32
_M32 = np.uint64(0xFFFFFFFF)


def hash32(v):
    v = np.asarray(v, dtype=np.uint64) & _M32      # 32-bit words in 64-bit lanes: products are masked, nothing overflows
    v = v ^ (v >> np.uint64(16))
    v = (v * np.uint64(0x7FEB352D)) & _M32
    v = v ^ (v >> np.uint64(15))
    v = (v * np.uint64(0x846CA68B)) & _M32
    v = v ^ (v >> np.uint64(16))
    return v


def round_keys(key):
    key = int(key) & (2 ** 64 - 1)
    klo, khi = key & 0xFFFFFFFF, key >> 32
    return [int(hash32(int(hash32((klo + r * 0x9E3779B9) & 0xFFFFFFFF)) ^ khi)) for r in range(ROUNDS)]


def feistel_bits(n_rays):
    bits = 2
    while (1 << bits) < n_rays:
        bits += 2
    return bits


def feistel(v, rk, half):
    v = np.asarray(v, dtype=np.uint64)
    mask = np.uint64((1 << half) - 1)
    L, R = v >> np.uint64(half), v & mask
    for r in range(ROUNDS):
        L, R = R, L ^ (hash32(R ^ np.uint64(rk[r])) & mask)
    return (L << np.uint64(half)) | R


def sigma(p, n_rays, order, key, return_walks=False):
    """int64 ray indices of the epoch positions ``p``; with ``return_walks`` also how often each was walked again."""
    p = np.asarray(p, dtype=np.int64)
    walks = np.zeros(p.shape, dtype=np.int64)
    if order == IDENTITY:
        out = p.copy()
    elif order == PERMUTED:
        rk, half = round_keys(key), feistel_bits(n_rays) // 2
        v = feistel(p.astype(np.uint64), rk, half)
        while True:
            again = v >= np.uint64(n_rays)
            if not again.any():
                break
            v[again] = feistel(v[again], rk, half)
            walks[again] += 1
        out = v.astype(np.int64)
    elif order == RANDOM:
        rk = round_keys(key)
        pu = p.astype(np.uint64)
        plo, phi = pu & _M32, pu >> np.uint64(32)
        a = hash32(hash32(plo ^ np.uint64(rk[0])) ^ phi ^ np.uint64(rk[1]))
        c = hash32(a ^ np.uint64(rk[2]))
        out = (((a << np.uint64(32)) | c) % np.uint64(n_rays)).astype(np.int64)
    else:
        raise ValueError(order)
    return (out, walks) if return_walks else out


def scaled_intrinsics(fx, fy, cx, cy, height, h):
    s = 1.0 / (float(height) / float(h))
    return tuple(F(float(v) * s) for v in (fx, fy, cx, cy))


def composite(images_u8, white_bkgd):
    """fp32 ``[n, H, W, 3]``: ``u8 / 255``, over white with an alpha channel and ``white_bkgd``."""
    q = images_u8.astype(F) / F(255.0)
    if images_u8.shape[-1] == 4:
        a = q[..., 3:]
        q = q[..., :3] * a + (F(1.0) - a) if white_bkgd else q[..., :3]
    return np.ascontiguousarray(q, dtype=F)


def area(q, h, w):
    """fp32 ``[n, h, w, 3]``: the mean over the windows of torch's ``mode="area"``, summed row by row, left to right."""
    n, H, W, _ = q.shape
    out = np.zeros((n, h, w, 3), dtype=F)
    for y in range(h):
        y0, y1 = (y * H) // h, ((y + 1) * H + h - 1) // h
        for x in range(w):
            x0, x1 = (x * W) // w, ((x + 1) * W + w - 1) // w
            s = np.zeros((n, 3), dtype=F)
            for yy in range(y0, y1):
                for xx in range(x0, x1):
                    s = s + q[:, yy, xx]
            out[:, y, x] = s / F((y1 - y0) * (x1 - x0))
    return out


def all_rays(images_u8, c2w, fx, fy, cx, cy, white_bkgd=True, factor=1):
    """``(origins, dirs, rgb)``, each fp32 ``[N, 3]``, of every ray of the epoch in index order ``(image * h + y) * w + x``."""
    images_u8 = np.asarray(images_u8)
    n, H, W, _ = images_u8.shape
    h, w = H // factor, W // factor
    pose = np.asarray(c2w, dtype=F).reshape(n, -1)[:, :12].reshape(n, 3, 4)
    fxs, fys, cxs, cys = scaled_intrinsics(fx, fy, cx, cy, H, h)
    u = ((np.arange(w, dtype=F) + F(0.5)) - cxs) / fxs
    v = ((np.arange(h, dtype=F) + F(0.5)) - cys) / fys
    u, v = np.broadcast_to(u[None, :], (h, w)), np.broadcast_to(v[:, None], (h, w))
    m = np.sqrt((u * u + v * v) + F(1.0))
    d = [(u / m).reshape(1, -1), (v / m).reshape(1, -1), (F(1.0) / m).reshape(1, -1)]
    dirs = np.stack([(pose[:, r, 0:1] * d[0] + pose[:, r, 1:2] * d[1]) + pose[:, r, 2:3] * d[2] for r in range(3)], -1)
    origins = np.broadcast_to(pose[:, None, :, 3], (n, h * w, 3))
    rgb = area(composite(images_u8, white_bkgd), h, w)
    return (np.ascontiguousarray(origins.reshape(-1, 3), dtype=F), np.ascontiguousarray(dirs.reshape(-1, 3), dtype=F),
            np.ascontiguousarray(rgb.reshape(-1, 3), dtype=F))


def batch(rays, order, key, begin, n):
    """``(origins, dirs, rgb, indices)`` of rows ``[begin, begin + n)`` of the epoch, from :func:`all_rays`' result."""
    idx = sigma(np.arange(begin, begin + n, dtype=np.int64), rays[0].shape[0], order, key)
    return rays[0][idx], rays[1][idx], rays[2][idx], idx
