"""Writes tests/golden/octree.npz: the reference's own spherical harmonics, as arrays.

    NERF_REFERENCE_PLENOCTREE=/path/to/reference/plenoctree python tests/golden/make_golden_octree.py

Runs ``eval_sh`` of the reference's ``nerf_sh/nerf/sh.py`` (it needs only numpy) in fp64 on 256 seeded unit directions and
random coefficients, for degrees 0 to 4. Only arrays are stored: ``dirs [256, 3]``, and per degree ``k`` the coefficients
``sh_k [256, 3, (k + 1)^2]`` and the result ``out_k [256, 3]``. tests/octree_oracle.py's basis must meet them to 1e-12
(test_octree_cpu.py); the kernels follow the oracle. Nothing else of the octree can be anchored on the reference: svox, which
holds the container and the march, is not part of it.
"""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    root = os.environ["NERF_REFERENCE_PLENOCTREE"]
    spec = importlib.util.spec_from_file_location("reference_sh", os.path.join(root, "nerf_sh", "nerf", "sh.py"))
    sh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sh)
    rng = np.random.default_rng(20250)
    v = rng.standard_normal((256, 3))
    dirs = v / np.linalg.norm(v, axis=1, keepdims=True)
    out = {"dirs": dirs}
    for deg in range(5):
        coeff = rng.standard_normal((256, 3, (deg + 1) ** 2))
        out[f"sh_{deg}"] = coeff
        out[f"out_{deg}"] = np.asarray(sh.eval_sh(deg, coeff, dirs), dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "octree.npz"), **out)
    print("wrote octree.npz", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
