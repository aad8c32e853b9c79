// The small launches of the training step with an occupancy grid (train_api.cpp, nerf_train_step_occ): what joins the list of
// kept points (occupancy_kernels.hip, launch_occ_compact) to the compact buffers the backward kernels read.
//   * occ_embed_kernel: gamma(x) / gamma(d) of the listed points, written at the list slots (the X operands of the weight
//     gradients), and the pass's sigma noise copied for the listed points only (nerf_mi355x.h, "Occupancy grid": a skipped
//     sample's alpha is exactly 0);
//   * occ_gather_rows_kernel: d raw of the listed points into list order (16 bytes per kept point and 4 channels);
//   * occ_scatter_rows_kernel: raw of a layer-by-layer forward pass, which ran on the compact rows, back to the [N, S] rows.
// Semantics: nerf_mi355x.h, "Occupancy grid"; route and costs: DESIGN.md 7c.
#include "nerf_internal.h"

namespace nerf {

// embed_train_kernel's expressions (train_kernels.hip: the same products, sums and sincosf calls per entry, so a list that
// names every point gives the dense step's encodings bit for bit) over slot n -> point index[n]. A workgroup takes 64 slots.
constexpr int kOccEmbedPoints = 64;
__global__ __launch_bounds__(256) void occ_embed_kernel(const float* __restrict__ rays, int ray_ld, const float* __restrict__ z,
                                                        const int* __restrict__ index, int M, int S, int Lx, int Lv,
                                                        float* __restrict__ x0, int ld0, float* __restrict__ x1, int ld1,
                                                        float* __restrict__ vcat, int ldv, int voff, int pad,
                                                        const float* __restrict__ noise_in, float* __restrict__ noise_out) {
    __shared__ float sx[kOccEmbedPoints][64];   // 3 + 6 Lx <= 63 columns
    __shared__ float sv[kOccEmbedPoints][28];   // 3 + 6 Lv <= 27 columns
    __shared__ float sz[kOccEmbedPoints];
    __shared__ int sray[kOccEmbedPoints];
    const int64_t p0 = (int64_t)blockIdx.x * kOccEmbedPoints;
    const int n_here = (int)((M - p0) < kOccEmbedPoints ? (M - p0) : kOccEmbedPoints);
    const int fx = Lx + 1, fv = Lv + 1;      // frequency slot 0 is the identity term
    if ((int)threadIdx.x < n_here) {
        const int pt = index[p0 + threadIdx.x];
        sz[threadIdx.x] = z[pt];
        sray[threadIdx.x] = pt / S;
        if (noise_out) noise_out[pt] = noise_in[pt];      // (every other entry of noise_out was zeroed by the caller)
    }
    __syncthreads();
    for (int it = threadIdx.x; it < kOccEmbedPoints * 3 * fx; it += 256) {
        const int pl = it / (3 * fx), c = (it / fx) % 3, k = it % fx - 1;
        if (pl >= n_here) continue;
        const float* r = rays + (int64_t)sray[pl] * ray_ld;
        const float p = __fadd_rn(r[c], __fmul_rn(r[3 + c], sz[pl]));   // nerf.ipynb:447
        if (k < 0) {
            sx[pl][c] = p;
        } else {
            float sn, cs;
            sincosf(p * (float)(1 << k), &sn, &cs);
            sx[pl][3 + 6 * k + c] = sn;
            sx[pl][3 + 6 * k + 3 + c] = cs;
        }
    }
    if (vcat)
        for (int it = threadIdx.x; it < kOccEmbedPoints * 3 * fv; it += 256) {
            const int pl = it / (3 * fv), c = (it / fv) % 3, k = it % fv - 1;
            if (pl >= n_here) continue;
            const float d = rays[(int64_t)sray[pl] * ray_ld + ray_ld - 3 + c];
            if (k < 0) {
                sv[pl][c] = d;
            } else {
                float sn, cs;
                sincosf(d * (float)(1 << k), &sn, &cs);
                sv[pl][3 + 6 * k + c] = sn;
                sv[pl][3 + 6 * k + 3 + c] = cs;
            }
        }
    __syncthreads();
    const int in_ch = 3 + 6 * Lx, in_v = 3 + 6 * Lv;
    const int w0 = pad ? ld0 : in_ch, wv = pad ? ldv - voff : in_v;      // (pad: rows zero-padded to their strides)
    for (int it = threadIdx.x; it < n_here * w0; it += 256) {
        const int pl = it / w0, col = it % w0;
        const float v = col < in_ch ? sx[pl][col] : 0.0f;
        x0[(p0 + pl) * ld0 + col] = v;
        if (x1 && col < in_ch) x1[(p0 + pl) * ld1 + col] = v;
    }
    if (vcat)
        for (int it = threadIdx.x; it < n_here * wv; it += 256) {
            const int pl = it / wv, col = it % wv;
            vcat[(p0 + pl) * ldv + voff + col] = col < in_v ? sv[pl][col] : 0.0f;
        }
}

hipError_t launch_occ_embed(const float* rays, int ray_ld, const float* z, const int* index, int64_t M, int S, int Lx, int Lv,
                            float* x0, int ld0, float* x1, int ld1, float* vcat, int ldv, int voff, int pad,
                            const float* noise_in, float* noise_out, hipStream_t s) {
    if (M <= 0) return hipSuccess;
    if (M > 0x7fffffffLL || S < 1 || Lx < 0 || Lx > 10 || Lv < 0 || Lv > 4 || !x0 || !index || (noise_out && !noise_in))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(occ_embed_kernel, dim3((unsigned)((M + kOccEmbedPoints - 1) / kOccEmbedPoints)), dim3(256), 0, s, rays,
                       ray_ld, z, index, (int)M, S, Lx, Lv, x0, ld0, x1, ld1, vcat, ldv, voff, pad, noise_in, noise_out);
    return hipGetLastError();
}

// dst[n][0..C) = src[index[n]][0..C): one thread per float (C is 4 or 8: a wavefront copies whole rows side by side)
__global__ __launch_bounds__(256) void occ_gather_rows_kernel(const float* __restrict__ src, const int* __restrict__ index,
                                                              int64_t n_floats, int C, float* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_floats) return;
    const int64_t n = i / C;
    const int c = (int)(i - n * C);
    dst[i] = src[(int64_t)index[n] * C + c];
}
__global__ __launch_bounds__(256) void occ_scatter_rows_kernel(const float* __restrict__ src, const int* __restrict__ index,
                                                               int64_t n_floats, int C, float* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_floats) return;
    const int64_t n = i / C;
    const int c = (int)(i - n * C);
    dst[(int64_t)index[n] * C + c] = src[i];
}

hipError_t launch_occ_gather_rows(const float* src, const int* index, int64_t M, int C, float* dst, hipStream_t s) {
    if (M <= 0 || C <= 0) return hipSuccess;
    if (!src || !index || !dst) return hipErrorInvalidValue;
    const int64_t n = M * C;
    hipLaunchKernelGGL(occ_gather_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, index, n, C, dst);
    return hipGetLastError();
}
hipError_t launch_occ_scatter_rows(const float* src, const int* index, int64_t M, int C, float* dst, hipStream_t s) {
    if (M <= 0 || C <= 0) return hipSuccess;
    if (!src || !index || !dst) return hipErrorInvalidValue;
    const int64_t n = M * C;
    hipLaunchKernelGGL(occ_scatter_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, index, n, C, dst);
    return hipGetLastError();
}

}  // namespace nerf
