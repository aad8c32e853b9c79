// Sparse voxel grid, the sparsity term of the Plenoxels objective as a value and its backward: the two ray kernels of
// "Sparse voxel grid: regularisers as values" (include/nerf_mi355x.h), instantiated by grid_regularisers_kernels.hip. Siblings
// of the depth kernels of grid_depth_autograd_kernels.hip on the same grid_march (grid_device.h), so the sample lattice, the
// thresholds, the stop and the skip rule are the renderer's by construction; densities only, no SH row is read. One lane per
// ray. The backward marches the ray again with the same log_T recurrence and adds to the 8 corner rows with
// atomicAdd(float*) = one global_atomic_add_f32 without return. Design: DESIGN.md section 7n.
#pragma once
#include "grid_device.h"

namespace nerf {
namespace {

template <bool SKIP>
__global__ __launch_bounds__(kGridThreads) void grid_sparsity_kernel(GridDev g, GridRenderOpt opt, GridSparsity r) {
    const int64_t ray = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (ray >= r.n_rays) return;
    GridRay rs;
    load_ray(r.origins, r.dirs, ray, rs);
    setup_ray<SKIP>(g, opt, rs);
    float total = 0.0f;
    if (rs.ok && rs.tmin <= rs.tmax) {
        const float neg_step = -opt.step_size;
        float log_t = 0.0f;
        grid_march<SKIP>(g, opt, rs, [&](float, const int*, const float*, const float*, float sigma) {
            if (!(sigma > opt.sigma_thresh)) return false;
            total = add(total, log1pf(mul(2.0f, mul(sigma, sigma))));
            log_t = add(log_t, mul(mul(neg_step, sigma), rs.delta_scale));
            return expf(log_t) < opt.stop_thresh;
        });
    }
    r.sparsity[ray] = total;
}

template <bool SKIP>
__global__ __launch_bounds__(kGridThreads) void grid_sparsity_bwd_kernel(GridDev g, GridRenderOpt opt, GridSparsity r) {
    const int64_t ray = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (ray >= r.n_rays) return;
    GridRay rs;
    load_ray(r.origins, r.dirs, ray, rs);
    setup_ray<SKIP>(g, opt, rs);
    if (!(rs.ok && rs.tmin <= rs.tmax)) return;      // a miss or a non-finite set-up: nothing to differentiate
    const float g_r = r.grad_sparsity[ray];
    if (g_r == 0.0f) return;      // every term would be zero
    const float neg_step = -opt.step_size;
    float log_t = 0.0f;
    grid_march<SKIP>(g, opt, rs, [&](float, const int* lk, const float* wa, const float* wb, float sigma) {
        if (!(sigma > opt.sigma_thresh)) return false;
        const float d_sigma = mul(g_r, __fdiv_rn(mul(4.0f, sigma), add(1.0f, mul(2.0f, mul(sigma, sigma)))));
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            if (lk[c] < 0) continue;
            const float v = mul(corner_weight(c, wa, wb), d_sigma);
            if (v != 0.0f) atomicAdd(&r.grad_density[lk[c]], v);
        }
        log_t = add(log_t, mul(mul(neg_step, sigma), rs.delta_scale));
        return expf(log_t) < opt.stop_thresh;
    });
}

}  // namespace
}  // namespace nerf
