"""When each workgroup of an inference MLP launch ends, and on which XCD (profiles/tile_claim_ab.md). The instrumentation is
not in the shipped sources: profiles/microbench/tile_end_stamps.patch adds it (to a copy of the tree, or take it out again).

    git apply profiles/microbench/tile_end_stamps.patch
    NERF_LIB_OUT=$PWD/nerf-projects_amd/libnerf_stamps.so python nerf-projects_amd/build.py --force
    NERF_MI355X_LIB=.../libnerf_stamps.so NERF_STAMPS_FILE=/tmp/stamps.bin python bench.py --gpus 1 --steps 3 --warmup 1
    python profiles/microbench/tile_end_stamps.py /tmp/stamps.bin

A record per workgroup and launch: s_memrealtime (100 MHz) at the kernel's start and end, s_memtime (shader cycles) between
the two, and a word with the XCD (HW_REG_XCC_ID), the tiles the workgroup claimed and the grid. The file is appended to every 40
launches (one 800 x 800 frame of 32 768-ray chunks); the first frame is the warm-up and is left out."""
import sys
import numpy as np

r = np.fromfile(sys.argv[1], dtype=np.uint64).reshape(-1, 256, 4)
for kind in ("coarse", "fine"):
    rows = []
    for L in r[40:]:
        t0, t1, cyc = L[:, 0].astype(np.int64), L[:, 1].astype(np.int64), L[:, 2].astype(np.float64)
        xcd, tiles = (L[:, 3] & 0xf).astype(int), ((L[:, 3] >> 8) & 0xffffff).astype(np.float64)
        end = (t1 - t0.min()) / 100.0      # us from the first workgroup's start
        if not ((3000.0 < end.max() < 6000.0) if kind == "coarse" else end.max() > 9000.0):      # (the frame's last chunk is a
            continue                                                                               # short one: neither)
        per = [(end[xcd == x].mean(), (cyc[xcd == x] / ((t1 - t0)[xcd == x] * 10.0)).mean(), tiles[xcd == x].mean()) for x in range(8)]
        rows.append((end.max(), 1.0 - end.mean() / end.max(), end.max() - end.min(), per))
    per = np.array([p for *_, p in rows]).mean(0)
    print(f"{kind}: {len(rows)} launches, {np.mean([x[0] for x in rows]):.1f} us; workgroups idle at the end "
          f"{100 * np.mean([x[1] for x in rows]):.2f} % of the launch; first to last end {np.mean([x[2] for x in rows]):.1f} us")
    for x in range(8):
        print(f"  XCD {x}: ends at {per[x, 0]:.1f} us, {per[x, 1]:.3f} GHz, {per[x, 2]:.1f} tiles claimed per workgroup")
