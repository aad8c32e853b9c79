// The claimed tile schedule of the inference MLP kernels (MlpLaunch::tile_claim; DESIGN 3.1, profiles/tile_claim_ab.md).
// Host and device: the sequence is plain integer arithmetic, so tests/test_tile_claim.py runs it on the CPU.
//
// A launch is `grid` persistent workgroups over `n_tiles` equal tiles; share = ceil(n_tiles / grid) is what the static loop
// gives each of them. The XCDs hold different clocks under this load, so with equal shares the launch ends with the slowest
// XCD. Claimed, a workgroup takes contiguous batches of tiles instead. Its first batch is its own by position (workgroup b:
// tiles [b * first, (b + 1) * first), no memory operation); every later one is [base + old, base + old + size) with `old`
// what one atomic add of `size` on the launch's counter returned and base = grid * first. A claim at or past n_tiles means
// leave; a batch is cut at n_tiles.
//
// The sizes depend on (share, tiles this workgroup has claimed so far) alone: one fixed decreasing sequence, the same for
// every workgroup - half of what is left up to `reach`, then single tiles. reach = share - share / 8: a workgroup that runs
// 12.5 % below the launch's mean pace is still on single tiles when the pool runs dry, so it ends at most one tile after the
// others (measured spread of the XCDs' clocks: +-4 %, one launch +-8 %). Faster workgroups take their surplus as
// single tiles.
#pragma once

#if defined(__HIPCC__)
#define NERF_TILE_CLAIM_HD __host__ __device__
#else
#define NERF_TILE_CLAIM_HD
#endif

namespace nerf {

NERF_TILE_CLAIM_HD inline int tile_claim_reach(int share) { return share - share / 8; }

// size of the batch a workgroup asks for when it has claimed `done` tiles so far (done = 0: the batch it owns by position)
NERF_TILE_CLAIM_HD inline int tile_claim_batch(int share, int done) {
    const int left = tile_claim_reach(share) - done;
    return left >= 4 ? left / 2 : 1;
}

// Atomic claims of a workgroup that ran `tiles` tiles are at most this: the batches of two tiles and more halve what is left
// up to reach (fewer than log2(share) + 1 of them, and together they stay below reach), single tiles for the rest, and the one
// claim that finds the pool dry. With workgroups within a few per cent of one pace that is log2(share) + share / 8 + a few.
NERF_TILE_CLAIM_HD inline int tile_claim_max_claims(int share, int tiles) {
    int halvings = 0, done = 0;
    for (int b = tile_claim_batch(share, 0); b > 1; b = tile_claim_batch(share, done)) {
        done += b;
        ++halvings;
    }
    const int singles = tiles > done ? tiles - done : 0;
    return (halvings > 0 ? halvings - 1 : 0) + singles + 1;      // (the first batch is not a claim)
}

}  // namespace nerf
