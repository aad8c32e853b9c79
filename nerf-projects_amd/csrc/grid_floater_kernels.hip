// Sparse voxel grid (Plenoxels): floater views - the labelled nodes of the connected components projected into a camera: the
// heatmap of visible floaters and the z-buffered component view. Semantics: include/nerf_mi355x.h, "Sparse voxel grid:
// floater views". Design and measurements: DESIGN.md section 7j.
//
// Both scans are one thread per node in C order (z fastest, so a wavefront reads 64 consecutive labels) and leave at the
// label: a node whose label is 0 or whose table entry is 0 reads nothing else, and that is the great majority. The only
// writes that race are integer atomics (atomicAdd on int32 counts, atomicMin on uint64 keys), whose results do not depend on
// the order of arrival: two calls give identical bits. Node counts reach 2^30, so flat thread indices are int64_t; a pixel
// index fits int32 (at most 2^26 pixels). No scratch, no LDS, no inline assembly, no float atomic, no compare-and-swap.
#include "grid_device.h"
#include "grid_floater_internal.h"

namespace nerf {
namespace {

// the node's table entry: 0 for label 0, a label outside [1, n_labels] or an entry of 0
__device__ __forceinline__ int32_t table_entry(const int32_t* __restrict__ labels, const int32_t* __restrict__ table,
                                               int64_t n_labels, int64_t idx) {
    const int32_t l = labels[idx];
    if (l <= 0 || (int64_t)l > n_labels) return 0;
    return table[l];
}

// The reference's projection of node (ix, iy, iz), fp32 with every operation rounded: p = ((idx / reso) * 2 - 1) * radius +
// center (the voxel's corner, not grid2world's centre), q = w2c [p, 1] summed left to right, x = (q0 / q2) * fx + cx.
// Returns whether the node is valid: q2 > 0, 0 <= x < width, 0 <= y < height (a NaN fails every comparison).
__device__ __forceinline__ bool project_node(const GridFloaterView& v, int64_t idx, float& q2, int& xi, int& yi) {
    int c[3];
    node_to_xyz(idx, v.size, c[0], c[1], c[2]);
    float p[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        p[k] = add(mul(sub(mul(__fdiv_rn((float)c[k], (float)v.size[k]), 2.0f), 1.0f), v.radius[k]), v.center[k]);
    float q[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
        q[r] = add(add(add(mul(v.w2c[r * 4 + 0], p[0]), mul(v.w2c[r * 4 + 1], p[1])), mul(v.w2c[r * 4 + 2], p[2])), v.w2c[r * 4 + 3]);
    const float x = add(mul(__fdiv_rn(q[0], q[2]), v.fx), v.cx);
    const float y = add(mul(__fdiv_rn(q[1], q[2]), v.fy), v.cy);
    q2 = q[2];
    const bool valid = q2 > 0.0f && x >= 0.0f && x < (float)v.width && y >= 0.0f && y < (float)v.height;
    xi = valid ? (int)x : 0;
    yi = valid ? (int)y : 0;
    return valid;
}

// One atomic per wavefront and counter: the lanes' flags summed by a ballot. Atomics on one address are served one after the
// other (measured: 25 000 wavefronts adding to three words took 0.5 ms at 128^3, the whole kernel), so the sums are spread over
// kFloaterCounterSlots slots, each on a 128-byte line of its own, chosen by the block; the dilation kernel adds the slots up.
__device__ __forceinline__ void count_flags(bool flag, int lane, int32_t* counter) {
    const unsigned long long set = __ballot(flag);
    if (lane == 0 && set != 0ull) atomicAdd(counter, (int32_t)__popcll(set));
}

// ---- heatmap: counts ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kGridThreads) void grid_floater_scan_kernel(GridFloaterView v, const int32_t* __restrict__ links,
                                                                          const float* __restrict__ density, int64_t capacity,
                                                                          GridFloaterHeat h) {
    const int64_t idx = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool cand = idx < v.nodes && table_entry(v.labels, v.table, v.n_labels, idx) != 0;
    if (!__any(cand)) return;      // (wavefront-uniform: the ballots below see every lane of a wavefront that stays)
    bool dense = cand;
    if (cand && h.use_density) {
        const int32_t l = links[idx];
        const float rho = (l >= 0 && (int64_t)l < capacity) ? density[l] : 0.0f;
        dense = rho >= h.min_density;
    }
    float q2 = 0.0f;
    int xi = 0, yi = 0;
    const bool in_view = dense && project_node(v, idx, q2, xi, yi) && xi < h.out_width && yi < h.out_height;
    bool visible = in_view;
    if (in_view && h.depth) {
        const float d = h.depth[yi * v.width + xi];
        visible = q2 < add(d, 0.05f) || d < 0.01f;
    }
    if (visible) atomicAdd(h.counts + (yi * h.out_width + xi), 1);
    int32_t* slot = h.counter_slots + (blockIdx.x % kFloaterCounterSlots) * kFloaterSlotStride;
    count_flags(dense, lane, slot + 0);
    count_flags(in_view, lane, slot + 1);
    count_flags(visible, lane, slot + 2);
}

// ---- heatmap: the 3 x 3 maximum over the in-image neighbours (cv2.dilate's default border), as float. Nothing decides whether
// any count is non-zero: the maximum over an all-zero image is that image. Block 0 also adds the counter slots up into
// counters[3] (zeroed before the launch): thread t takes slot t, a wavefront sums by shuffles, four integer adds per counter.
__global__ __launch_bounds__(kGridThreads) void grid_floater_dilate_kernel(GridFloaterHeat h) {
    static_assert(kFloaterCounterSlots == kGridThreads, "one thread of block 0 per slot");
    if (blockIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            int32_t v = h.counter_slots[threadIdx.x * kFloaterSlotStride + k];
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
            if ((threadIdx.x & 63) == 0 && v != 0) atomicAdd(h.counters + k, v);
        }
    }
    const int pix = (int)((int64_t)blockIdx.x * kGridThreads + threadIdx.x);
    if (pix >= h.out_width * h.out_height) return;
    const int y = pix / h.out_width, x = pix % h.out_width;
    int32_t m = 0;
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= h.out_height) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = x + dx;
            if (xx < 0 || xx >= h.out_width) continue;
            m = max(m, h.counts[yy * h.out_width + xx]);
        }
    }
    h.heatmap[pix] = (float)m;
}

// ---- component view: the smallest (q2, slot) key of the nodes whose disc dx^2 + dy^2 <= 5 covers a pixel ---------------------------
__global__ __launch_bounds__(kGridThreads) void grid_component_scan_kernel(GridFloaterView v, unsigned long long* __restrict__ keys) {
    const int64_t idx = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (idx >= v.nodes) return;
    const int32_t slot = table_entry(v.labels, v.table, v.n_labels, idx);
    if (slot <= 0) return;
    float q2;
    int xi, yi;
    if (!project_node(v, idx, q2, xi, yi)) return;
    // q2 > 0: the bit pattern orders as the float does
    const unsigned long long key = ((unsigned long long)__float_as_uint(q2) << 32) | (unsigned long long)(uint32_t)slot;
    for (int dy = -2; dy <= 2; ++dy) {
        const int yy = yi + dy;
        if (yy < 0 || yy >= v.height) continue;
        for (int dx = -2; dx <= 2; ++dx) {
            const int xx = xi + dx;
            if (dx * dx + dy * dy > 5 || xx < 0 || xx >= v.width) continue;
            // (a plain load of the key first, to skip the atomic behind something nearer, was measured: 1.44x slower at
            // 128^3, 0.95x at 256^3 - the load's latency comes before every atomic; not kept)
            atomicMin(keys + (yy * v.width + xx), key);
        }
    }
}

__global__ __launch_bounds__(kGridThreads) void grid_component_resolve_kernel(const unsigned long long* __restrict__ keys, int n,
                                                                               int32_t* __restrict__ slots) {
    const int pix = (int)((int64_t)blockIdx.x * kGridThreads + threadIdx.x);
    if (pix >= n) return;
    const unsigned long long k = keys[pix];
    slots[pix] = k == ~0ull ? 0 : (int32_t)(k & 0xffffffffull);
}

}  // namespace

hipError_t launch_grid_floater_heatmap(const GridDev& g, const GridFloaterView& v, const GridFloaterHeat& h, hipStream_t s) {
    const int pixels = h.out_width * h.out_height;
    hipError_t e = hipMemsetAsync(h.counts, 0, (size_t)pixels * sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(h.counters, 0, 3 * sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(h.counter_slots, 0, (size_t)kFloaterCounterSlots * kFloaterSlotStride * sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(grid_floater_scan_kernel, dim3(blocks_for(v.nodes)), dim3(kGridThreads), 0, s, v, g.links, g.density,
                       g.capacity, h);
    hipLaunchKernelGGL(grid_floater_dilate_kernel, dim3(blocks_for(pixels)), dim3(kGridThreads), 0, s, h);
    return hipGetLastError();
}

hipError_t launch_grid_component_view(const GridFloaterView& v, unsigned long long* keys, int32_t* slots, hipStream_t s) {
    const int pixels = v.width * v.height;
    hipError_t e = hipMemsetAsync(keys, 0xff, (size_t)pixels * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(grid_component_scan_kernel, dim3(blocks_for(v.nodes)), dim3(kGridThreads), 0, s, v, keys);
    hipLaunchKernelGGL(grid_component_resolve_kernel, dim3(blocks_for(pixels)), dim3(kGridThreads), 0, s, keys, pixels, slots);
    return hipGetLastError();
}

}  // namespace nerf
