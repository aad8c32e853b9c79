"""The claimed tile schedule's batch sequence (nerf-projects_amd/csrc/tile_claim.h) on the CPU.

The header is plain integer arithmetic shared by host and device. A small C++ program includes it and plays a launch of 256
persistent workgroups that run at unequal speeds - an event queue ordered by the time at which a workgroup reaches its next
tile boundary, one shared counter, the claim protocol of mlp_kernel_h2_body.inc word for word (first batch by position, later
batches [base + old, base + old + size), leave at or past the end). For every tile count it prints what the test asserts:

* every tile is run exactly once and none at or past the end;
* a workgroup's atomic claims stay within tile_claim_max_claims(share, tiles it ran) - and, with speeds a few per cent
  apart, within log2(share) + share / 8 + 6 plus the fastest die's surplus over the share (the single tiles of the tail);
* with the XCDs' speeds up to +-8 % apart (MI355X: +-3 % in steady state, +-8 % in a process's first launches) every
  workgroup that ran the tail ends within one tile of the last one, and the launch ends no later than the static split's.

With speeds +-30 % apart only the first two are asserted: the sequence is built for dies of one chip."""
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nerf-projects_amd", "csrc")

SIM = r"""
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <queue>
#include <vector>
#include "tile_claim.h"
using namespace nerf;

struct Wg { double t, cost; long tile, end; int done, claims, ran; bool left; };

int main(int argc, char** argv) {
    const long n = atol(argv[1]);
    const int grid = atoi(argv[2]);
    const double spread = atof(argv[3]);      // die b % 8 runs a tile in 1 + spread * (b % 8 - 3.5) / 3.5, +-0.5 % per workgroup
    const int share = (int)((n + grid - 1) / grid);
    const int first = tile_claim_batch(share, 0);
    const long base = (long)grid * first;
    std::vector<int> taken(n, 0);
    std::vector<Wg> w(grid);
    long counter = 0, past_end = 0;
    unsigned rng = 12345u;
    typedef std::pair<double, int> Ev;
    std::priority_queue<Ev, std::vector<Ev>, std::greater<Ev>> q;
    double static_end = 0.0, slowest = 0.0;
    for (int b = 0; b < grid; ++b) {
        rng = rng * 1664525u + 1013904223u;
        const double jitter = ((int)((rng >> 8) % 1001u) - 500) * 1e-5;
        w[b].cost = (1.0 + spread * ((b % 8) - 3.5) / 3.5) * (1.0 + jitter);
        slowest = std::max(slowest, w[b].cost);
        static_end = std::max(static_end, w[b].cost * (double)((n - b + grid - 1) / grid));      // tiles b, b + grid, ...
        w[b].t = 0.0;
        w[b].tile = (long)b * first;
        w[b].end = std::min(w[b].tile + first, n);
        w[b].done = first;
        w[b].claims = w[b].ran = 0;
        w[b].left = false;
        q.push(Ev(0.0, b));
    }
    while (!q.empty()) {
        const int b = q.top().second;
        q.pop();
        Wg& g = w[b];
        if (g.tile >= g.end) {      // a tile boundary with the batch used up: claim
            const int size = tile_claim_batch(share, g.done);
            const long old = counter;
            counter += size;
            ++g.claims;
            g.tile = base + old;
            if (g.tile >= n) { g.left = true; continue; }
            g.end = std::min(g.tile + size, n);
            g.done += size;
        }
        if (g.tile >= n) { ++past_end; g.left = true; continue; }
        ++taken[g.tile];
        ++g.tile;
        ++g.ran;
        g.t += g.cost;
        q.push(Ev(g.t, b));
    }
    long once = 0;
    for (long i = 0; i < n; ++i) once += taken[i] == 1;
    int over_bound = 0, max_claims = 0, min_ran = 1 << 30, max_ran = 0, all_left = 1;
    double end_max = 0.0, tail_min = 1e300;
    for (int b = 0; b < grid; ++b) {
        over_bound += w[b].claims > tile_claim_max_claims(share, w[b].ran);
        max_claims = std::max(max_claims, w[b].claims);
        min_ran = std::min(min_ran, w[b].ran);
        max_ran = std::max(max_ran, w[b].ran);
        all_left &= w[b].left || w[b].tile >= w[b].end;
        end_max = std::max(end_max, w[b].t);
    }
    for (int b = 0; b < grid; ++b)
        if (w[b].claims > 1) tail_min = std::min(tail_min, w[b].t);      // took part in the tail (more than the claim that failed)
    if (tail_min > end_max) tail_min = end_max;
    printf("%ld %d %ld %ld %d %d %d %d %d %.6f %.6f %.6f %.6f\n", n, share, once, past_end, over_bound, max_claims, min_ran,
           max_ran, all_left, end_max, tail_min, static_end, slowest);
    return 0;
}
"""

TILES = (257, 1027, 16384, 49152, 255, 256, 513, 4099, 30011, 65537)


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    d = tmp_path_factory.mktemp("tile_claim")
    src = d / "sim.cpp"
    src.write_text(SIM)
    exe = d / "sim"
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def run(n, grid, spread):
        out = subprocess.run([str(exe), str(n), str(grid), str(spread)], check=True, capture_output=True, text=True).stdout.split()
        keys = ("n", "share", "once", "past_end", "over_bound", "max_claims", "min_ran", "max_ran", "all_left", "end_max",
                "tail_min", "static_end", "slowest")
        return {k: (float(v) if "." in v else int(v)) for k, v in zip(keys, out)}
    return run


@pytest.mark.parametrize("spread", [0.0, 0.03, 0.08, 0.30])
@pytest.mark.parametrize("n", TILES)
def test_every_tile_once_and_claims_bounded(sim, n, spread):
    r = sim(n, 256, spread)
    print(r)
    assert r["n"] == n and r["share"] == (n + 255) // 256
    assert r["once"] == n, "a tile was skipped or run twice"
    assert r["past_end"] == 0
    assert r["all_left"] == 1
    assert r["over_bound"] == 0
    if spread <= 0.08:
        # halvings, the single tiles from reach to the share, the fastest die's surplus over the share, and a few
        log2 = max(r["share"], 1).bit_length() - 1
        surplus = math.ceil(r["share"] * (1.0 / (1.0 - spread) - 1.0))
        assert r["max_claims"] <= log2 + r["share"] // 8 + surplus + 6, r
        # the tail is single tiles: who took part in it ends within one (slowest) tile of the end
        assert r["end_max"] - r["tail_min"] <= r["slowest"] + 1e-9, r
        assert r["end_max"] <= r["static_end"] + 1e-9, r


@pytest.mark.parametrize("n", (16384, 49152))
def test_balance_recovers_the_spread(sim, n):
    """Dies +-3 % apart, the bench's launches: static ends with the slowest die (3 % behind the mean); claimed ends within one
    tile and the claims' granularity of the mean pace."""
    r = sim(n, 256, 0.03)
    ideal = n / 256.0      # mean tile time 1, every workgroup busy to the end
    assert r["static_end"] >= 1.025 * ideal
    assert r["end_max"] <= ideal + 1.5 * r["slowest"], (r, ideal)


def test_sequence_is_decreasing_and_reaches_single_tiles():
    """The same arithmetic restated: sizes never grow, the multi-tile batches stay below reach = share - share / 8."""
    for share in (1, 2, 3, 4, 5, 7, 8, 9, 64, 65, 192, 257, 1000):
        reach = share - share // 8
        done, prev, sizes = 0, None, []
        while True:
            left = reach - done
            b = left // 2 if left >= 4 else 1
            sizes.append(b)
            assert prev is None or b <= prev
            if b == 1:
                break
            done += b
            prev = b
        assert done <= reach and len(sizes) <= max(share, 2).bit_length() + 1, (share, sizes)
