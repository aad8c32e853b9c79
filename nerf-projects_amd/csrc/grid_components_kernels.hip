// Sparse voxel grid (Plenoxels): connected components of the occupied nodes, for floater detection and removal - occupancy,
// union-find labelling, relabelling in C order, component volumes, the keep mask of a removal and the bit-exact row copy.
// Semantics: include/nerf_mi355x.h, "Sparse voxel grid: connected components". Design and measurements: DESIGN.md section 7f.
//
// The labelling is a label-equivalence union-find over one int32 parent per node. A parent is never larger than its node, a
// component's root is its smallest flat index, and the only writes that race are atomicMin, so the result does not depend on
// the order of arrival: two calls give identical bits. Node counts reach 2^30, so a node index fits int32; flat thread
// indices are int64_t. No scratch, no inline assembly, no float atomic, no compare-and-swap; LDS only in the root count / rank
// (compact_device.h: 16 ballots per workgroup and the one-workgroup scan). Every pointer-chasing loop has an iteration cap that
// sets the error word instead of spinning.
#include "compact_device.h"
#include "grid_device.h"

namespace nerf {
namespace {

constexpr int kChaseCap = 1 << 22;        // steps of one find, and rounds of one union, before the error word is set

// ---- occupancy: one thread per node -----------------------------------------------------------------------------------------
// kept and, with use_density, density > threshold in fp32 (NaN is not occupied); any negative link is empty
__global__ __launch_bounds__(kGridThreads) void grid_occupancy_kernel(const int32_t* __restrict__ links,
                                                                       const float* __restrict__ density, int64_t n, int64_t capacity,
                                                                       int use_density, float threshold, uint8_t* __restrict__ occ) {
    const int64_t idx = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (idx >= n) return;
    const int32_t l = links[idx];
    bool o = l >= 0 && (int64_t)l < capacity;
    if (o && use_density) o = density[l] > threshold;
    occ[idx] = o ? 1 : 0;
}

// ---- union-find ------------------------------------------------------------------------------------------------------------
// A wavefront holds 64 consecutive nodes of C order, so a run of occupied nodes along z is a run of set bits of the ballot,
// cut where a new z row starts. Every node of a run starts with the run's first node as its parent: inside a run no union is
// needed, and only the first node of a run that continues a run of the wavefront before it has to be linked to it.
__global__ __launch_bounds__(kGridThreads) void grid_label_init_kernel(const uint8_t* __restrict__ occ, int64_t n, int sz,
                                                                        int32_t* __restrict__ parent) {
    const int64_t idx = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool o = idx < n && occ[idx] != 0;
    const int z = (int)(idx % sz);
    const unsigned long long set = __ballot(o);
    const bool head = o && (lane == 0 || z == 0 || !((set >> (lane - 1)) & 1ull));
    const unsigned long long heads = __ballot(head);
    if (!o) return;      // (the parent of an empty node is never read)
    const unsigned long long at_or_below = heads & ((2ull << lane) - 1ull);      // (lane 63: 2 << 63 wraps to 0, all bits)
    const int head_lane = 63 - __clzll(at_or_below);
    parent[idx] = (int32_t)(idx - (lane - head_lane));
}

// The root of x. Within the merging launch a load of a parent may be stale (the XCDs' L2s are not coherent with each other
// and a CU's L1 is not refreshed by another CU's atomics): parents only decrease and every value a parent ever held is a
// member of the node's component, so a stale parent is an older, larger ancestor - the walk takes more steps or stops at a
// node that is no longer a root, and never leaves the component. The relaxed agent-scope loads only make stale values rarer.
// With `halve`, every second node of the path is pointed at its grandparent by an atomicMin whose result is not used.
template <bool halve>
__device__ __forceinline__ int find_root(int32_t* parent, int x, int32_t* err) {
    for (int it = 0; it < kChaseCap; ++it) {
        const int p = halve ? __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : parent[x];
        if (p == x) return x;
        if (p < 0 || p > x) {      // not a parent this file can have written
            *err = 2;
            return -1;
        }
        if (!halve) {
            x = p;
            continue;
        }
        const int g = __hip_atomic_load(parent + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (g == p) return p;
        if (g < 0 || g > p) {
            *err = 2;
            return -1;
        }
        atomicMin(parent + x, g);
        x = g;
    }
    *err = 1;
    return -1;
}

// Joins the components of a and b. Correctness rests only on what atomicMin RETURNS, which is the parent's true value:
//   a, b = the (possibly stale) roots found, a > b.  old = atomicMin(&parent[a], b).
//   old == a: a was a root and now points at b - joined.
//   old <  a: a had already been given the parent old (the load that called it a root was stale, or another lane won). Its
//             parent is now min(old, b), so one of the two edges a - old, a - b is stored and the other is what is left to
//             do: the loop goes on with the pair (old, b). old < a, so the pair decreases strictly and the loop ends.
// A stale load therefore costs rounds, never a wrong or a lost union.
__device__ __forceinline__ void unite(int32_t* parent, int a, int b, int32_t* err) {
    for (int it = 0; it < kChaseCap; ++it) {
        a = find_root<true>(parent, a, err);
        b = find_root<true>(parent, b, err);
        if (a < 0 || b < 0 || a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(parent + a, b);
        if (old == a) return;
        if (old < 0 || old > a) {
            *err = 2;
            return;
        }
        a = old;
    }
    *err = 1;
}

// One thread per node; an occupied node is joined to its occupied neighbours in the rows BEFORE it in C order (the other half
// of the neighbourhood is the neighbours' job). Per earlier row (dx, dy) the three candidates z - 1, z, z + 1 are themselves
// a z run, and so are this node and its z neighbours, so most of the contacts say nothing new:
//   centre occupied: one union with it - unless this node's z - 1 neighbour and the row's z - 1 node are both occupied, in
//                    which case that neighbour (same run as this node) meets the same run of the row and does it;
//   centre empty:    z - 1 only when this node's own z - 1 neighbour is empty (else the centre rule of that neighbour does it),
//                    z + 1 only when this node's own z + 1 neighbour is empty (likewise).
// conn 6: rows (-1, 0) and (0, -1), centre only. conn 18: those two rows with z +- 1, rows (-1, -1) and (-1, +1) centre only.
// conn 26: all four rows with z +- 1. No wrap-around: a row outside the lattice is skipped.
__global__ __launch_bounds__(kGridThreads) void grid_label_merge_kernel(const uint8_t* __restrict__ occ, int sx, int sy, int sz,
                                                                         int conn, int32_t* parent, int32_t* err) {
    const int64_t n = (int64_t)sx * sy * sz;
    const int64_t idx = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (idx >= n || occ[idx] == 0) return;
    const int i = (int)idx;
    const int z = i % sz, y = (i / sz) % sy, x = i / (sz * sy);
    const bool below = z > 0 && occ[i - 1] != 0, above = z < sz - 1 && occ[i + 1] != 0;
    // a run cut by the wavefront boundary (the init kernel started a new run at lane 0)
    if ((threadIdx.x & 63) == 0 && below) unite(parent, i, i - 1, err);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int dx = r == 3 ? 0 : -1, dy = r == 0 ? -1 : r == 1 ? 0 : r == 2 ? 1 : -1;
        const bool face_row = r == 1 || r == 3;      // the row differs in one coordinate only
        if (!face_row && conn == 6) continue;
        if (x + dx < 0 || y + dy < 0 || y + dy >= sy) continue;
        const bool with_z = conn == 26 || (conn == 18 && face_row);
        const int j = i + dx * sy * sz + dy * sz;
        if (occ[j] != 0) {
            if (!(below && occ[j - 1] != 0)) unite(parent, i, j, err);
        } else if (with_z) {
            if (z > 0 && !below && occ[j - 1] != 0) unite(parent, i, j - 1, err);
            if (z < sz - 1 && !above && occ[j + 1] != 0) unite(parent, i, j + 1, err);
        }
    }
}

// A later launch (so every parent of the merge is visible): every occupied node gets its root as its parent, and the roots
// are counted per workgroup (the count launch of compact_device.h). Nodes are rewritten while other lanes still walk through them; a walker then sees the old parent
// or the root, both ancestors, and a root's own entry never changes here.
__global__ __launch_bounds__(kGridThreads) void grid_label_flatten_kernel(const uint8_t* __restrict__ occ, int64_t n, int32_t* parent,
                                                                           int32_t* __restrict__ block_offsets, int32_t* err) {
    int roots = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t node = compact_item(r);
        bool is_root = false;
        if (node < n && occ[node] != 0) {
            const int root = find_root<false>(parent, (int)node, err);
            if (root >= 0) {
                if (root != (int)node) parent[node] = root;
                is_root = root == (int)node;
            }
        }
        roots += __popcll(__ballot(is_root));
    }
    compact_store_count(roots, block_offsets);
}

// one workgroup turns the per-workgroup counts into exclusive offsets (in place) and stores the total
__global__ __launch_bounds__(1024) void grid_label_scan_kernel(int32_t* counts, int64_t n, int32_t* total) {
    const int v = compact_scan(counts, n);
    if (threadIdx.x == 1023) *total = v;
}

// labels[root] = 1 + the number of roots before it in C order (no atomics: the numbering is that of the lattice)
__global__ __launch_bounds__(kGridThreads) void grid_label_rank_kernel(const uint8_t* __restrict__ occ, int64_t n,
                                                                        const int32_t* __restrict__ parent,
                                                                        const int32_t* __restrict__ block_offsets,
                                                                        int32_t* __restrict__ labels) {
    bool is_root[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t node = compact_item(r);
        is_root[r] = node < n && occ[node] != 0 && parent[node] == (int32_t)node;
    }
    const CompactRanks ranks = compact_ranks(is_root, block_offsets);
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (is_root[r]) labels[compact_item(r)] = 1 + ranks.rank(r);
}

// every other node: its root's label, or 0 when it is not occupied (a root's own entry is left as the rank kernel wrote it)
__global__ __launch_bounds__(kGridThreads) void grid_label_spread_kernel(const uint8_t* __restrict__ occ, int64_t n,
                                                                          const int32_t* __restrict__ parent, int32_t* labels) {
    const int64_t idx = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (idx >= n) return;
    if (occ[idx] == 0) {
        labels[idx] = 0;
        return;
    }
    const int32_t root = parent[idx];
    if (root == (int32_t)idx) return;
    labels[idx] = root >= 0 && root < (int32_t)idx ? labels[root] : 0;      // (a parent the flatten could not resolve: error word set)
}

// ---- volumes: an integer histogram of the labels ----------------------------------------------------------------------------
// Equal labels sit next to each other along z: the first lane of every stretch of equal labels in the wavefront adds the
// stretch's length, one atomic per stretch instead of one per node. The result is not used, the sum does not depend on order.
__global__ __launch_bounds__(kGridThreads) void grid_label_volumes_kernel(const int32_t* __restrict__ labels, int64_t n, int64_t count,
                                                                           int32_t* volumes) {
    const int64_t idx = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int32_t label = idx < n ? labels[idx] : 0;
    const int32_t before = __shfl_up(label, 1);
    const bool first = lane == 0 || before != label;
    const unsigned long long firsts = __ballot(first);
    if (!first || label <= 0 || (int64_t)label > count) return;
    const unsigned long long above = lane == 63 ? 0ull : firsts >> (lane + 1);
    const int length = above ? __ffsll((long long)above) : 64 - lane;
    atomicAdd(volumes + (label - 1), length);
}

// ---- removal ---------------------------------------------------------------------------------------------------------------
// a kept node stays unless its component is marked; label 0 (kept but not occupied) always stays
__global__ __launch_bounds__(kGridThreads) void grid_keep_mask_kernel(const int32_t* __restrict__ links, const int32_t* __restrict__ labels,
                                                                       int64_t n, const uint8_t* __restrict__ floater, int64_t count,
                                                                       uint8_t* __restrict__ mask) {
    const int64_t idx = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (idx >= n) return;
    const int32_t label = labels[idx];
    const bool marked = label > 0 && (int64_t)label <= count && floater[label - 1] != 0;
    mask[idx] = links[idx] >= 0 && !marked ? 1 : 0;
}

// src_row[new link] = old link, for the nodes the new grid keeps
__global__ __launch_bounds__(kGridThreads) void grid_row_sources_kernel(const int32_t* __restrict__ old_links,
                                                                         const int32_t* __restrict__ new_links, int64_t n, int64_t old_rows,
                                                                         int64_t new_rows, int32_t* __restrict__ src_row) {
    const int64_t idx = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (idx >= n) return;
    const int32_t to = new_links[idx], from = old_links[idx];
    if (to >= 0 && (int64_t)to < new_rows && from >= 0 && (int64_t)from < old_rows) src_row[to] = from;
}

// one thread per (row, column) of [density | sh]: 32-bit words are moved, not floats, so that every bit pattern survives
__global__ __launch_bounds__(kGridThreads) void grid_copy_rows_kernel(const int32_t* __restrict__ src_row, int64_t new_rows, int64_t old_rows,
                                                                       int cols, const uint32_t* __restrict__ old_density,
                                                                       const uint32_t* __restrict__ old_sh, uint32_t* __restrict__ density,
                                                                       uint32_t* __restrict__ sh) {
    const int64_t tid = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    const int64_t row = tid / (cols + 1);
    const int j = (int)(tid % (cols + 1));
    if (row >= new_rows) return;
    const int64_t from = src_row[row];
    if (from < 0 || from >= old_rows) return;      // (links that are no sub-selection of the old ones: nothing is read)
    if (j == cols)
        density[row] = old_density[from];
    else
        sh[row * cols + j] = old_sh[from * cols + j];
}

}  // namespace

hipError_t launch_grid_occupancy(const GridDev& g, int use_density, float threshold, uint8_t* occ, hipStream_t s) {
    const int64_t n = (int64_t)g.size[0] * g.size[1] * g.size[2];
    grid_occupancy_kernel<<<blocks_for(n), kGridThreads, 0, s>>>(g.links, g.density, n, g.capacity, use_density, threshold, occ);
    return hipGetLastError();
}

hipError_t launch_grid_label(const GridLabel& a, hipStream_t s) {
    const int64_t n = (int64_t)a.size[0] * a.size[1] * a.size[2];
    const int64_t nb = compact_blocks(n);
    hipError_t e = hipMemsetAsync(a.status, 0, 2 * sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    grid_label_init_kernel<<<blocks_for(n), kGridThreads, 0, s>>>(a.occ, n, a.size[2], a.parent);
    grid_label_merge_kernel<<<blocks_for(n), kGridThreads, 0, s>>>(a.occ, a.size[0], a.size[1], a.size[2], a.connectivity, a.parent,
                                                                   a.status + 1);
    grid_label_flatten_kernel<<<(unsigned)nb, kGridThreads, 0, s>>>(a.occ, n, a.parent, a.block_offsets, a.status + 1);
    grid_label_scan_kernel<<<1, 1024, 0, s>>>(a.block_offsets, nb, a.status);
    grid_label_rank_kernel<<<(unsigned)nb, kGridThreads, 0, s>>>(a.occ, n, a.parent, a.block_offsets, a.labels);
    grid_label_spread_kernel<<<blocks_for(n), kGridThreads, 0, s>>>(a.occ, n, a.parent, a.labels);
    return hipGetLastError();
}

hipError_t launch_grid_label_volumes(const int32_t* labels, int64_t n, int64_t count, int32_t* volumes, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(volumes, 0, (size_t)count * sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    grid_label_volumes_kernel<<<blocks_for(n), kGridThreads, 0, s>>>(labels, n, count, volumes);
    return hipGetLastError();
}

hipError_t launch_grid_keep_mask(const int32_t* links, const int32_t* labels, int64_t n, const uint8_t* floater, int64_t count,
                                 uint8_t* mask, hipStream_t s) {
    grid_keep_mask_kernel<<<blocks_for(n), kGridThreads, 0, s>>>(links, labels, n, floater, count, mask);
    return hipGetLastError();
}

hipError_t launch_grid_copy_rows(const GridCopyRows& a, hipStream_t s) {
    if (a.new_rows <= 0) return hipSuccess;
    // a row no link names copies row 0 of the old tables (which exist: new_rows > 0 needs old_rows > 0)
    hipError_t e = hipMemsetAsync(a.src_row, 0, (size_t)a.new_rows * sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    grid_row_sources_kernel<<<blocks_for(a.nodes), kGridThreads, 0, s>>>(a.old_links, a.new_links, a.nodes, a.old_rows, a.new_rows, a.src_row);
    grid_copy_rows_kernel<<<blocks_for(a.new_rows * (a.cols + 1)), kGridThreads, 0, s>>>(
        a.src_row, a.new_rows, a.old_rows, a.cols, reinterpret_cast<const uint32_t*>(a.old_density),
        reinterpret_cast<const uint32_t*>(a.old_sh), reinterpret_cast<uint32_t*>(a.density), reinterpret_cast<uint32_t*>(a.sh));
    return hipGetLastError();
}

}  // namespace nerf
