"""numpy restatement of the NDC warp of forward-facing scenes (include/nerf_mi355x.h, rays_to_ndc): svox2's
``convert_to_ndc`` with ``near = 1`` and the normalisation after it, every operation rounded to fp32, in the reference's
order. The fused multiply-adds of the norm are evaluated exactly in fp64 and rounded once: a product of two fp32 values is
exact in fp64, and the sum of such a product and an fp32 (or another exact product's fp32 rounding) is rounded to fp64 first
and to fp32 second. A double rounding could differ from a true fma only where the fp64 sum lands exactly on an fp32 tie,
which needs the discarded fp64 bits to matter at 2^-29 relative: the fixture has no such case, and the test that compares
this file with the reference's bits would show one."""
import numpy as np

F = np.float32


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def rays_to_ndc(origins, dirs, ndc_coeffs):
    """fp32 ``[n, 3]`` origins and dirs -> fp32 ``[n, 3]`` NDC origins and unit dirs."""
    o = np.asarray(origins, dtype=F)
    d = np.asarray(dirs, dtype=F)
    cx, cy = F(ndc_coeffs[0]), F(ndc_coeffs[1])
    with np.errstate(all="ignore"):
        t = (F(1.0) - o[:, 2]) / d[:, 2]
        o = o + t[:, None] * d                      # a product, then a sum (numpy rounds each)
        ox, oy, two_oz = o[:, 0] / o[:, 2], o[:, 1] / o[:, 2], F(2.0) / o[:, 2]
        dx = cx * (d[:, 0] / d[:, 2] - ox)
        dy = cy * (d[:, 1] / d[:, 2] - oy)
        n = np.sqrt(_fma(two_oz, two_oz, _fma(dy, dy, dx * dx)))
        oo = np.stack([cx * ox, cy * oy, F(1.0) - two_oz], -1)
        dd = np.stack([dx / n, dy / n, two_oz / n], -1)
    assert oo.dtype == F and dd.dtype == F
    return oo, dd
