// Sparse voxel grid (Plenoxels): training data - a batch of rays (origin, direction, ground-truth colour) made from the
// resident uint8 images and poses. Semantics: include/nerf_mi355x.h, "Sparse voxel grid: training data". Design and
// measurements: DESIGN.md section 7o.
//
// One lane per output row k: the ray index sigma(begin + k), its image / pixel, the direction of svox2's gen_rays in rounded
// fp32 operations, the translation column as the origin (both through rays_to_ndc of grid_device.h where the data set has
// ndc_coeffs: a forward-facing scene), and the composited colour of the pixel (factor 1) or the mean over its area window
// (factor > 1). The kernel is a gather: in the permuted and random orders neighbouring lanes read pixels of
// different images, 3 or 4 bytes each (one 32-bit load with an alpha channel), and the twelve pose floats of their image; the
// three [n, 3] outputs are stored row by row, so a wavefront writes 768 contiguous bytes per output. Row and pixel arithmetic
// is int64_t (n_images * height * width may pass 2^31). No LDS, no scratch, no atomics, no inline assembly.
//
// The permuted order walks cycles: feistel() is a bijection of [0, 2^bits) with 2^bits < 4 N, and a walk that starts at
// p < N stays on p's cycle, which contains p, so `while (v >= N)` comes back into [0, N) after finitely many steps (fewer than
// 4 on average; the longest walk seen is recorded by tests/test_grid_dataset_cpu.py). Lanes of a wavefront walk different
// lengths: the loop runs to the longest of the 64.
#include "grid_dataset_internal.h"
#include "grid_device.h"

namespace nerf {
namespace {

// four balanced Feistel rounds on `2 * half` bits
__device__ __forceinline__ int64_t feistel(const GridDatasetBatch& b, int64_t v) {
    const uint32_t mask = (1u << b.half) - 1u;
    uint32_t L = (uint32_t)(v >> b.half), R = (uint32_t)v & mask;
#pragma unroll
    for (int r = 0; r < kDatasetRounds; ++r) {
        const uint32_t t = L ^ (hash32(R ^ b.rk[r]) & mask);
        L = R;
        R = t;
    }
    return ((int64_t)L << b.half) | (int64_t)R;
}

__device__ __forceinline__ int64_t sigma(const GridDatasetBatch& b, int64_t p) {
    if (b.order == NERF_GRID_ORDER_IDENTITY) return p;
    if (b.order == NERF_GRID_ORDER_PERMUTED) {
        int64_t v = feistel(b, p);
        while (v >= b.n_rays) v = feistel(b, v);
        return v;
    }
    const uint32_t plo = (uint32_t)p, phi = (uint32_t)((uint64_t)p >> 32);
    const uint32_t a = hash32(hash32(plo ^ b.rk[0]) ^ phi ^ b.rk[1]);
    const uint32_t c = hash32(a ^ b.rk[2]);
    return (int64_t)((((uint64_t)a << 32) | (uint64_t)c) % (uint64_t)b.n_rays);
}

// the composited colour of full-resolution pixel `pix` (flat over images, rows and columns)
__device__ __forceinline__ void pixel_colour(const GridDatasetBatch& b, int64_t pix, float q[3]) {
    if (b.channels == 4) {
        const uint32_t word = *reinterpret_cast<const uint32_t*>(b.images + pix * 4);
        const float a = __fdiv_rn((float)(word >> 24), 255.0f);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = __fdiv_rn((float)((word >> (8 * c)) & 255u), 255.0f);
            q[c] = b.white_bkgd ? add(mul(v, a), sub(1.0f, a)) : v;
        }
    } else {
        const uint8_t* p = b.images + pix * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) q[c] = __fdiv_rn((float)p[c], 255.0f);
    }
}

__global__ __launch_bounds__(kGridThreads) void grid_dataset_batch_kernel(GridDatasetBatch b) {
    const int64_t k = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (k >= b.n) return;
    const int64_t idx = sigma(b, b.begin + k);
    const int64_t per_image = (int64_t)b.h * b.w;
    const int64_t image = idx / per_image;
    const int64_t rest = idx - image * per_image;
    const int y = (int)(rest / b.w), x = (int)(rest - (int64_t)y * b.w);

    // direction: svox2's gen_rays, every operation rounded
    const float u = __fdiv_rn(sub(add((float)x, 0.5f), b.cx), b.fx);
    const float v = __fdiv_rn(sub(add((float)y, 0.5f), b.cy), b.fy);
    // sqrtf: the correctly rounded root (hipcc's default); __fsqrt_rn is the 1-ulp native root unless OCML's rounded operations are on
    const float m = sqrtf(add(add(mul(u, u), mul(v, v)), 1.0f));
    const float d0 = __fdiv_rn(u, m), d1 = __fdiv_rn(v, m), d2 = __fdiv_rn(1.0f, m);
    const float* pose = b.c2w + image * 12;
    float o[3], d[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        d[r] = add(add(mul(pose[4 * r], d0), mul(pose[4 * r + 1], d1)), mul(pose[4 * r + 2], d2));
        o[r] = pose[4 * r + 3];
    }
    // svox2's LLFFDataset.gen_rays: the world ray through the NDC warp (grid_device.h); the same branch for every lane
    if (b.ndc[0] > 0.0f) rays_to_ndc(b.ndc[0], b.ndc[1], o, d);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        b.dirs[k * 3 + r] = d[r];
        b.origins[k * 3 + r] = o[r];
    }

    // colour: the mean over the pixel's area window (one pixel at factor 1: 0 + q and q / 1 are exact)
    const int y0 = (int)(((int64_t)y * b.height) / b.h), y1 = (int)((((int64_t)y + 1) * b.height + b.h - 1) / b.h);
    const int x0 = (int)(((int64_t)x * b.width) / b.w), x1 = (int)((((int64_t)x + 1) * b.width + b.w - 1) / b.w);
    float sum[3] = {0.0f, 0.0f, 0.0f};
    for (int yy = y0; yy < y1; ++yy) {
        const int64_t row = (image * b.height + yy) * b.width;
        for (int xx = x0; xx < x1; ++xx) {
            float q[3];
            pixel_colour(b, row + xx, q);
#pragma unroll
            for (int c = 0; c < 3; ++c) sum[c] = add(sum[c], q[c]);
        }
    }
    const float count = (float)((y1 - y0) * (x1 - x0));
#pragma unroll
    for (int c = 0; c < 3; ++c) b.rgb[k * 3 + c] = __fdiv_rn(sum[c], count);
    if (b.indices) b.indices[k] = idx;
}

}  // namespace

hipError_t launch_grid_dataset_batch(const GridDatasetBatch& b, hipStream_t s) {
    if (b.n == 0) return hipSuccess;
    hipLaunchKernelGGL(grid_dataset_batch_kernel, dim3(blocks_for(b.n)), dim3(kGridThreads), 0, s, b);
    return hipGetLastError();
}

}  // namespace nerf
