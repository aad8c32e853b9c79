// Balanced median cut of order `bits` over [m, 3] fp32 colours: the quantiser behind the palette grid. The algorithm is stated in
// include/nerf_mi355x.h, "Sparse voxel grid: palette-quantised colours" (the reference calls a C extension of svox whose source
// is not available; the rule is this project's own, pinned by the numpy oracle of the tests). DESIGN.md 7p.
//
// The members live in one array `perm` in box order. A box's place in it is a pure function of (m, level, j) - box_of() below -
// so no scan and no host read is needed between levels. One level:
//   extents   min and max per box and axis, as atomicMin / atomicMax on sign-flipped bit patterns (order-independent, exact);
//             a wavefront whose 64 positions lie in one box reduces by shuffles first and issues 6 atomics, not 384
//   keys      key[p] = box << 32 | flipped bits of the member's value on the box's widest axis (ties: the lowest axis)
//   sort      hipCUB's stable DeviceRadixSort of (key, member) over the low 32 + level bits
// then every box's mean (fp64, one wavefront per box, lanes strided and a fixed shuffle tree: the same bits on every run) and
// the scatter of the box number to ids[member].
#include <hipcub/hipcub.hpp>

#include "grid_device.h"

namespace nerf {
namespace {

// the box of position p at `level`, its first position and its size: at each level a box of n members gives its first
// n - n / 2 to box 2 j and the other n / 2 to box 2 j + 1
struct Box {
    int64_t j, first, n;
};
__device__ __forceinline__ Box box_of(int64_t m, int level, int64_t p) {
    Box b{0, 0, m};
    for (int l = 0; l < level; ++l) {
        const int64_t lo = b.n - b.n / 2;
        if (p - b.first < lo) {
            b.j = 2 * b.j;
            b.n = lo;
        } else {
            b.j = 2 * b.j + 1;
            b.first += lo;
            b.n = b.n / 2;
        }
    }
    return b;
}
// the first position and the size of box j at `level` (j's bits from the top are the path)
__device__ __forceinline__ Box box_at(int64_t m, int level, int64_t j) {
    Box b{j, 0, m};
    for (int l = level - 1; l >= 0; --l) {
        const int64_t lo = b.n - b.n / 2;
        if ((j >> l) & 1) {
            b.first += lo;
            b.n = b.n / 2;
        } else {
            b.n = lo;
        }
    }
    return b;
}

// fp32 -> uint32 whose unsigned order is the order of the values, -0.0 below +0.0
__device__ __forceinline__ uint32_t flip(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unflip(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__global__ __launch_bounds__(kGridThreads) void median_cut_init_kernel(const float* __restrict__ colors, int64_t m,
                                                                        int32_t* __restrict__ perm, unsigned long long* nonfinite) {
    const int64_t i = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (i >= m) return;
    perm[i] = (int32_t)i;
    if (!(isfinite(colors[i * 3]) && isfinite(colors[i * 3 + 1]) && isfinite(colors[i * 3 + 2]))) atomicAdd(nonfinite, 1ull);
}

// minmax [boxes, 3, 2]: min starts at 0xffffffff, max at 0
__global__ __launch_bounds__(kGridThreads) void median_cut_reset_kernel(uint32_t* __restrict__ minmax, int64_t pairs) {
    const int64_t i = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (i >= pairs) return;
    minmax[2 * i] = 0xffffffffu;
    minmax[2 * i + 1] = 0u;
}

__global__ __launch_bounds__(kGridThreads) void median_cut_extent_kernel(const float* __restrict__ colors, int64_t m, int level,
                                                                          const int32_t* __restrict__ perm,
                                                                          uint32_t* __restrict__ minmax) {
    const int64_t p = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    const bool valid = p < m;
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    int64_t j = -1;
    if (valid) {
        j = box_of(m, level, p).j;
        const int64_t i = perm[p];
#pragma unroll
        for (int a = 0; a < 3; ++a) lo[a] = hi[a] = flip(colors[i * 3 + a]);
    }
    // (a workgroup is 4 whole wavefronts and no lane has left: the shuffles below see all 64 lanes)
    const int64_t j0 = __shfl(j, 0);      // lane 0 of a wavefront that reaches here with any valid lane is valid
    if (__all(!valid || j == j0)) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lo[a] = min(lo[a], (uint32_t)__shfl_xor((int)lo[a], off));
                hi[a] = max(hi[a], (uint32_t)__shfl_xor((int)hi[a], off));
            }
        if ((threadIdx.x & 63) != 0 || j0 < 0) return;
    } else if (!valid) {
        return;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        atomicMin(&minmax[(j * 3 + a) * 2], lo[a]);
        atomicMax(&minmax[(j * 3 + a) * 2 + 1], hi[a]);
    }
}

__global__ __launch_bounds__(kGridThreads) void median_cut_key_kernel(const float* __restrict__ colors, int64_t m, int level,
                                                                       const int32_t* __restrict__ perm,
                                                                       const uint32_t* __restrict__ minmax,
                                                                       unsigned long long* __restrict__ keys) {
    const int64_t p = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (p >= m) return;
    const Box b = box_of(m, level, p);
    uint32_t key = 0;      // a box of one member is not reordered
    if (b.n >= 2) {
        int axis = 0;
        float widest = -1.0f;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float extent = sub(unflip(minmax[(b.j * 3 + a) * 2 + 1]), unflip(minmax[(b.j * 3 + a) * 2]));
            if (extent > widest) {      // strictly: a tie stays with the lower axis
                widest = extent;
                axis = a;
            }
        }
        key = flip(colors[(int64_t)perm[p] * 3 + axis]);
    }
    keys[p] = ((unsigned long long)b.j << 32) | key;
}

constexpr int kWave = 64;

// one wavefront per final box: palette[j] = half(float(sum / n)), ids[member] = j
__global__ __launch_bounds__(kGridThreads) void median_cut_finish_kernel(const float* __restrict__ colors, int64_t m, int bits,
                                                                          const int32_t* __restrict__ perm,
                                                                          uint16_t* __restrict__ ids, uint16_t* __restrict__ palette) {
    const int64_t j = ((int64_t)blockIdx.x * kGridThreads + threadIdx.x) / kWave;
    const int lane = threadIdx.x % kWave;
    if (j >= ((int64_t)1 << bits)) return;      // (whole wavefronts leave)
    const Box b = box_at(m, bits, j);
    // (from -0.0, the identity of addition: a box of -0.0 members keeps its sign, and with one member a box the entry is half(x))
    double sum[3] = {-0.0, -0.0, -0.0};
    for (int64_t t = lane; t < b.n; t += kWave) {
        const int64_t i = perm[b.first + t];
        ids[i] = (uint16_t)j;
#pragma unroll
        for (int a = 0; a < 3; ++a) sum[a] += (double)colors[i * 3 + a];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int a = 0; a < 3; ++a) sum[a] += __shfl_down(sum[a], off);
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            float mean = b.n > 0 ? (float)(sum[a] / (double)b.n) : 0.0f;
            mean = fminf(fmaxf(mean, -65504.0f), 65504.0f);
            palette[j * 3 + a] = __builtin_bit_cast(uint16_t, (_Float16)mean);      // round to nearest even
        }
    }
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace

// the workspace: keys [2][m] uint64, perm [2][m] int32, minmax [2^(bits-1), 3, 2] uint32, the sort's own
void grid_median_cut_layout(int64_t m, int bits, GridMedianCutLayout* l) {
    const size_t mm = (size_t)m;
    l->keys = 0;
    l->perm = l->keys + align256(2 * mm * 8);
    l->minmax = l->perm + align256(2 * mm * 4);
    l->minmax_bytes = ((size_t)1 << (bits - 1)) * 6 * 4;
    l->nonfinite = l->minmax + align256(l->minmax_bytes);
    l->sort = l->nonfinite + 256;
    // rocPRIM's radix sort on caller-provided double buffers keeps histograms (a few KiB) and, in its onesweep form, one
    // look-back word per digit and block of at least 256 items: at most 8 bytes an item. The call checks the real figure.
    l->sort_bytes = 8 * mm + ((size_t)1 << 20);
    l->total = l->sort + l->sort_bytes;
}

hipError_t launch_grid_median_cut_count(const GridMedianCut& a, const GridMedianCutLayout& l, hipStream_t s) {
    char* ws = (char*)a.workspace;
    hipError_t e = hipMemsetAsync(ws + l.nonfinite, 0, 8, s);
    if (e != hipSuccess || a.m <= 0) return e;
    median_cut_init_kernel<<<blocks_for(a.m), kGridThreads, 0, s>>>(a.colors, a.m, (int32_t*)(ws + l.perm),
                                                                    (unsigned long long*)(ws + l.nonfinite));
    return hipGetLastError();
}

hipError_t launch_grid_median_cut(const GridMedianCut& a, const GridMedianCutLayout& l, hipStream_t s) {
    char* ws = (char*)a.workspace;
    const size_t mm = (size_t)a.m;
    unsigned long long* keys = (unsigned long long*)(ws + l.keys);
    int32_t* perm = (int32_t*)(ws + l.perm);
    uint32_t* minmax = (uint32_t*)(ws + l.minmax);
    hipcub::DoubleBuffer<unsigned long long> dk(keys, keys + mm);
    hipcub::DoubleBuffer<int32_t> dv(perm, perm + mm);      // perm[0] was filled by launch_grid_median_cut_count
    hipError_t e = hipSuccess;
    if (a.m >= 2) {
        for (int level = 0; level < a.bits; ++level) {
            if (a.m <= ((int64_t)1 << level)) break;      // every box has at most one member, now and from here on
            const int64_t pairs = ((int64_t)1 << level) * 3;
            median_cut_reset_kernel<<<blocks_for(pairs), kGridThreads, 0, s>>>(minmax, pairs);
            median_cut_extent_kernel<<<blocks_for(a.m), kGridThreads, 0, s>>>(a.colors, a.m, level, dv.Current(), minmax);
            median_cut_key_kernel<<<blocks_for(a.m), kGridThreads, 0, s>>>(a.colors, a.m, level, dv.Current(), minmax, dk.Current());
            e = hipGetLastError();
            if (e != hipSuccess) return e;
            size_t need = 0;
            e = hipcub::DeviceRadixSort::SortPairs(nullptr, need, dk, dv, (int)a.m, 0, 32 + level, s);
            if (e != hipSuccess) return e;
            if (need > l.sort_bytes) return hipErrorOutOfMemory;
            need = l.sort_bytes;
            e = hipcub::DeviceRadixSort::SortPairs(ws + l.sort, need, dk, dv, (int)a.m, 0, 32 + level, s);
            if (e != hipSuccess) return e;
        }
    }
    const int64_t boxes = (int64_t)1 << a.bits;
    median_cut_finish_kernel<<<blocks_for(boxes * kWave), kGridThreads, 0, s>>>(a.colors, a.m, a.bits, dv.Current(), a.ids, a.palette);
    return hipGetLastError();
}

}  // namespace nerf
