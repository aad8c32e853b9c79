// Occupancy grid: construction of the packed bit field and the per-pass classify + compact steps that let the fused
// encode+MLP kernels run over the kept points only (kInputRaysIndexed). Semantics: nerf_mi355x.h, "Occupancy grid".
//
// Nothing here waits for another workgroup of the same launch, and nothing appends with atomics: the kept points' ids
// come out in increasing order (count per workgroup, scan, scatter - three launches), so the fp16-pair kernel, which
// takes its scales per wavefront, sees the same wavefronts from run to run. The only atomic is the integer count of
// occupied cells at construction (order-independent).
#include "compact_device.h"
#include "mlp_inputs.h"

namespace nerf {

// ---- the cell rule ------------------------------------------------------------------------------------
// keep = the point needs the network. NaN / infinite positions are kept (the reference's NaN must still come out); a
// point is inside the box iff c1 <= p <= c2 on every axis (fp32); its cell on an axis is min(floor((p - c1) / cell),
// nc - 1) with the subtraction and the division each rounded to fp32 - the min puts the upper faces into the last cell.
__device__ __forceinline__ bool occ_keep_point(const OccGrid& g, const float (&p)[3]) {
    if (nonfinite(p[0]) || nonfinite(p[1]) || nonfinite(p[2])) return true;
    int idx[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!(p[a] >= g.c1[a] && p[a] <= g.c2[a])) return g.outside_keep != 0;
        const int i = (int)floorf(__fdiv_rn(__fsub_rn(p[a], g.c1[a]), g.cell[a]));
        idx[a] = i < g.nc[a] - 1 ? i : g.nc[a] - 1;
    }
    const uint32_t w = g.bits[((int64_t)idx[0] * g.nc[1] + idx[1]) * g.wz + (idx[2] >> 5)];
    return (w >> (idx[2] & 31)) & 1u;
}

// ---- classify: one thread per (ray, sample) -----------------------------------------------------------
// The count launch of the compaction (compact_device.h) over the points; the classification is the expensive part, so the
// 16 ballots of workgroup b are left in keep_words[b * 16 ..] for the scatter. The last sample of every ray is kept whatever
// the grid says (its dists is 1e10: nerf.ipynb:300). Rows of skipped points are zeroed here.
__global__ __launch_bounds__(256) void occ_classify_kernel(const OccCompact o) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t P = o.N * o.S;
    const bool vec = o.C == 4 && (reinterpret_cast<uintptr_t>(o.raw) & 15) == 0;      // (uniform)
    int kept = 0;
    for (int r = 0; r < 4; ++r) {
        const int64_t pt = compact_item(r);
        bool keep = false;
        if (pt < P) {
            const int64_t ray = pt / o.S;
            const int i = (int)(pt - ray * o.S);
            keep = i == o.S - 1;
            if (!keep) {
                // pts = rays_o + rays_d * z as the MLP kernels round it (mlp_inputs.h: product and sum separately)
                const float* rr = o.rays + ray * o.ray_ld;
                const float z = o.z[pt];
                float p[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) p[c] = __fadd_rn(rr[c], __fmul_rn(rr[3 + c], z));
                keep = occ_keep_point(o.g, p);
            }
            if (!keep) {
                if (vec) {
                    *(f32x4*)(o.raw + pt * 4) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                } else {
                    for (int c = 0; c < o.C; ++c) o.raw[pt * o.C + c] = 0.0f;
                }
            }
        }
        const unsigned long long ballot = __ballot(keep);
        if (lane == 0) o.keep_words[(int64_t)blockIdx.x * 16 + r * 4 + wave] = ballot;
        kept += __popcll(ballot);
    }
    compact_store_count(kept, o.block_counts);
}

// ---- scan: one workgroup turns the per-workgroup counts into exclusive offsets (in place) ---------------
__global__ __launch_bounds__(1024) void occ_scan_kernel(int* counts, int64_t n, int* total, unsigned long long* stats,
                                                        unsigned long long n_points) {
    const int v = compact_scan(counts, n);
    if (threadIdx.x == 1023) {
        *total = v;
        if (stats) {      // (stream-ordered launches of one thread each: no atomics needed)
            stats[0] += (unsigned long long)v;
            stats[1] += n_points;
        }
    }
}

// ---- scatter: ids of the kept points, in increasing order ---------------------------------------------
__global__ __launch_bounds__(256) void occ_scatter_kernel(const OccCompact o) {
    const CompactRanks ranks = compact_ranks(o.keep_words + (int64_t)blockIdx.x * 16, o.block_counts);
    for (int r = 0; r < 4; ++r)
        if (ranks.kept(r)) o.index[ranks.rank(r)] = (int)compact_item(r);
}

hipError_t launch_occ_compact(const OccCompact& o, hipStream_t s) {
    const int64_t P = o.N * o.S;
    if (P <= 0) return hipSuccess;
    if (P > 0x7fffffffLL || !o.keep_words || !o.block_counts || !o.index || !o.count || !o.g.bits) return hipErrorInvalidValue;
    const int64_t nb = compact_blocks(P);
    hipLaunchKernelGGL(occ_classify_kernel, dim3((unsigned)nb), dim3(256), 0, s, o);
    hipLaunchKernelGGL(occ_scan_kernel, dim3(1), dim3(1024), 0, s, o.block_counts, nb, o.count, o.stats, (unsigned long long)P);
    hipLaunchKernelGGL(occ_scatter_kernel, dim3((unsigned)nb), dim3(256), 0, s, o);
    return hipGetLastError();
}

// ---- construction -------------------------------------------------------------------------------------
constexpr int kOccMaxLattices = 8;
struct OccLattices {
    const float* sigma[kOccMaxLattices];
    int n;
};

// cell (i, j, k) is occupied when sigma at any of its 8 corner nodes is > threshold or NaN, in any lattice; a caller's byte
// mask is ORed in. One thread per cell, C order over [X-1, Y-1, Z-1].
__global__ __launch_bounds__(256) void occ_corner_kernel(const OccLattices L, const uint8_t* cell_mask, int ncx, int ncy, int ncz,
                                                         float threshold, uint8_t* out) {
    const int64_t n = (int64_t)ncx * ncy * ncz;
    const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (cell >= n) return;
    const int k = (int)(cell % ncz);
    const int64_t ij = cell / ncz;
    const int j = (int)(ij % ncy), i = (int)(ij / ncy);
    bool occ = cell_mask && cell_mask[cell] != 0;
    const int64_t Y = ncy + 1, Z = ncz + 1;
    for (int l = 0; l < L.n && !occ; ++l) {
        const float* sg = L.sigma[l];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float v = sg[((int64_t)(i + (c >> 2)) * Y + (j + ((c >> 1) & 1))) * Z + (k + (c & 1))];
            occ |= v > threshold || v != v;
        }
    }
    out[cell] = occ ? 1 : 0;
}

// one round of growth by a cell in all 26 directions
__global__ __launch_bounds__(256) void occ_dilate_kernel(const uint8_t* in, int ncx, int ncy, int ncz, uint8_t* out) {
    const int64_t n = (int64_t)ncx * ncy * ncz;
    const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (cell >= n) return;
    const int k = (int)(cell % ncz);
    const int64_t ij = cell / ncz;
    const int j = (int)(ij % ncy), i = (int)(ij / ncy);
    bool occ = false;
    for (int di = -1; di <= 1; ++di)
        for (int dj = -1; dj <= 1; ++dj)
            for (int dk = -1; dk <= 1; ++dk) {
                const int a = i + di, b = j + dj, c = k + dk;
                if (a >= 0 && a < ncx && b >= 0 && b < ncy && c >= 0 && c < ncz)
                    occ |= in[((int64_t)a * ncy + b) * ncz + c] != 0;
            }
    out[cell] = occ ? 1 : 0;
}

// 64 cells along z per wavefront: one ballot = two words of the bit field. Grid: (rows / 4, ceil(ncz / 64))
__global__ __launch_bounds__(256) void occ_pack_kernel(const uint8_t* in, int64_t rows, int ncz, int wz, uint32_t* bits,
                                                       unsigned long long* n_occupied) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;
    if (row >= rows) return;      // (whole wavefronts leave: the ballot below is over 64 lanes of one row)
    const int k = blockIdx.y * 64 + lane;
    const bool occ = k < ncz && in[row * ncz + k] != 0;
    const unsigned long long ballot = __ballot(occ);
    const int w0 = blockIdx.y * 2;
    if (lane == 0) bits[row * wz + w0] = (uint32_t)ballot;
    if (lane == 32 && w0 + 1 < wz) bits[row * wz + w0 + 1] = (uint32_t)(ballot >> 32);
    if (lane == 0 && ballot) atomicAdd(n_occupied, (unsigned long long)__popcll(ballot));
}

__global__ __launch_bounds__(256) void occ_unpack_kernel(const uint32_t* bits, int64_t n, int ncz, int wz, uint8_t* out) {
    const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (cell >= n) return;
    const int k = (int)(cell % ncz);
    const int64_t row = cell / ncz;
    out[cell] = (bits[row * wz + (k >> 5)] >> (k & 31)) & 1u;
}

hipError_t launch_occ_build(const float* const* sigma, int n_lattices, const uint8_t* cell_mask, const int32_t nc[3],
                            float threshold, int dilate, uint8_t* tmp0, uint8_t* tmp1, uint32_t* bits,
                            unsigned long long* n_occupied, hipStream_t s) {
    if (n_lattices < 0 || n_lattices > kOccMaxLattices || (n_lattices == 0 && !cell_mask) || dilate < 0) return hipErrorInvalidValue;
    OccLattices L{};
    L.n = n_lattices;
    for (int l = 0; l < n_lattices; ++l) {
        if (!sigma || !sigma[l]) return hipErrorInvalidValue;
        L.sigma[l] = sigma[l];
    }
    const int64_t n = (int64_t)nc[0] * nc[1] * nc[2];
    const unsigned blocks = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(occ_corner_kernel, dim3(blocks), dim3(256), 0, s, L, cell_mask, nc[0], nc[1], nc[2], threshold, tmp0);
    uint8_t *cur = tmp0, *other = tmp1;
    for (int d = 0; d < dilate; ++d) {
        hipLaunchKernelGGL(occ_dilate_kernel, dim3(blocks), dim3(256), 0, s, cur, nc[0], nc[1], nc[2], other);
        uint8_t* t = cur;
        cur = other;
        other = t;
    }
    const int wz = (nc[2] + 31) / 32;
    const int64_t rows = (int64_t)nc[0] * nc[1];
    hipError_t e = hipMemsetAsync(n_occupied, 0, sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(occ_pack_kernel, dim3((unsigned)((rows + 3) / 4), (unsigned)((nc[2] + 63) / 64)), dim3(256), 0, s, cur, rows,
                       nc[2], wz, bits, n_occupied);
    return hipGetLastError();
}

hipError_t launch_occ_unpack(const uint32_t* bits, const int32_t nc[3], uint8_t* mask, hipStream_t s) {
    const int64_t n = (int64_t)nc[0] * nc[1] * nc[2];
    hipLaunchKernelGGL(occ_unpack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, bits, n, nc[2], (nc[2] + 31) / 32, mask);
    return hipGetLastError();
}

}  // namespace nerf
