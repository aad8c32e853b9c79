// Sparse voxel grid (Plenoxels): the NDC warp of forward-facing scenes on a caller's own rays. Semantics:
// include/nerf_mi355x.h, "Sparse voxel grid" (rays_to_ndc, nerf_grid_rays_to_ndc); design: DESIGN.md section 7r.
//
// The warp itself is the device function rays_to_ndc of grid_device.h, which camera_ray (every image kernel, gen_rays, the
// weight render) and the data set's batch kernel inline; this file only gives it a kernel of its own. One lane per ray:
// 24 bytes in, 24 bytes out, five divisions and a root. A wavefront reads and writes 768 contiguous bytes per array. No LDS,
// no scratch, no atomics, no inline assembly.
#include "grid_device.h"

namespace nerf {
namespace {

// one lane per ray; an output may be its own input (no __restrict__): a lane has read its ray before it stores it
__global__ __launch_bounds__(kGridThreads) void grid_rays_to_ndc_kernel(const float* origins, const float* dirs, int64_t n,
                                                                         float coeffx, float coeffy, float* origins_out,
                                                                         float* dirs_out) {
    const int64_t ray = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (ray >= n) return;
    float o[3], d[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        o[i] = origins[ray * 3 + i];
        d[i] = dirs[ray * 3 + i];
    }
    rays_to_ndc(coeffx, coeffy, o, d);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        origins_out[ray * 3 + i] = o[i];
        dirs_out[ray * 3 + i] = d[i];
    }
}

}  // namespace

hipError_t launch_grid_rays_to_ndc(const float* origins, const float* dirs, int64_t n, float coeffx, float coeffy,
                                   float* origins_out, float* dirs_out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    grid_rays_to_ndc_kernel<<<blocks_for(n), kGridThreads, 0, s>>>(origins, dirs, n, coeffx, coeffy, origins_out, dirs_out);
    return hipGetLastError();
}

}  // namespace nerf
