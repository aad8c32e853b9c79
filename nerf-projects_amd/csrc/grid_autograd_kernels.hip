// Sparse voxel grid, gradients for autograd: the two marches of grid_fused_kernel (grid_train_kernels.hip) as kernels of their
// own, with the cotangent d loss / d rgb read from memory between them, and the transpose of grid_sample_kernel. Semantics:
// include/nerf_mi355x.h, "Sparse voxel grid: gradients for autograd". Design, generated-code figures and measurements:
// DESIGN.md section 7h.
//
// Both render kernels keep the lane layout of grid_render_kernel (grid_device.h, group_lane): one SH coefficient per lane, a
// ray owns a group of 32 / 16 / 4 lanes at basis_dim 9 / 4 / 1, control flow uniform inside a group. grid_taped_kernel calls
// march_colour (grid_device.h), the function grid_fused_kernel's first march calls, and leaves, besides the colour, the tape:
// per ray and channel the colour as the fp64 sum of its exact weight * colour products plus the background term (24 B per
// ray). grid_render_bwd_kernel calls march_colour_bwd, the fused kernel's second march: `remaining` starts from the tape,
// g_c comes from grad_rgb, and at every shaded sample lane (c, k) adds w8 * (weight * Y_k * g_c) to grad_sh[row, c * B + k]
// while lanes 0..7 of the group (0..3 twice at basis_dim 1) each take one corner's density add and mask byte. A table whose
// pointer is NULL gets nothing: the test is uniform over the launch.
// Float adds are atomicAdd(float*) = one global_atomic_add_f32 without return (no compare-and-swap loop); the mask is
// written with plain byte stores (every writer stores 1). No LDS, no scratch.
// grid_render_bwd_kernel is written in grid_train_device.h; this file instantiates it without the loss terms,
// grid_train_losses_kernels.hip with.
#include "grid_train_device.h"

namespace nerf {
namespace {

template <int B, bool SKIP>
__global__ __launch_bounds__(kGridThreads) void grid_taped_kernel(GridDev g, GridRenderOpt opt, GridTaped r) {
    const GroupLane gl = group_lane<B>();
    if (gl.ray >= r.n_rays) return;
    GridRay rs;
    load_ray(r.origins, r.dirs, gl.ray, rs);
    setup_ray<SKIP>(g, opt, rs);
    const float yk = gl.busy ? sh_basis(gl.k, rs.v[0], rs.v[1], rs.v[2]) : 0.0f;
    const Colour c = march_colour<B, SKIP, true, false>(g, opt, rs, gl, yk);
    if (gl.busy && gl.k == 0) {      // the lanes in which the channel's sum is complete
        r.rgb[gl.ray * 3 + gl.col / B] = c.outv;
        r.tape[gl.ray * 3 + gl.col / B] = c.tot;
    }
    if (gl.lane == 0 && r.log_transmit) r.log_transmit[gl.ray] = c.log_t;
}

// The transpose of grid_sample_kernel: one thread per (point, column), column 0 = density. The cell, the weights and the
// world -> grid transform are that kernel's; corner (x, y, z bits) of a kept link receives ((w_x * go) * w_y) * w_z.
__global__ __launch_bounds__(kGridThreads) void grid_sample_bwd_kernel(GridDev g, GridSampleBwd a, int cols) {
    const int64_t tid = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    const int64_t p = tid / cols;
    const int j = (int)(tid % cols);
    if (p >= a.n) return;
    const int row = 3 * g.basis_dim;
    float* table = j == 0 ? a.grad_density : a.grad_sh;
    if (!table) return;
    const float go = j == 0 ? a.grad_out_density[p] : a.grad_out_sh[p * row + (j - 1)];
    float x[3], wa[3], wb[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        x[i] = a.points[p * 3 + i];
        if (!a.grid_coords) x[i] = add(g.offset[i], mul(x[i], g.scaling[i]));
    }
    int lk[8];
    load_links(g, point_cell(g, x, wa, wb), lk);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        if (lk[c] < 0) continue;
        const float v = mul(mul(mul((c & 4) ? wb[0] : wa[0], go), (c & 2) ? wb[1] : wa[1]), (c & 1) ? wb[2] : wa[2]);
        if (v != 0.0f) atomicAdd(j == 0 ? &table[lk[c]] : &table[(int64_t)lk[c] * row + (j - 1)], v);
    }
}

}  // namespace

hipError_t launch_grid_render_taped(const GridDev& g, const GridRenderOpt& o, const GridTaped& r, hipStream_t s) {
    if (r.n_rays <= 0) return hipSuccess;
    return dispatch_basis(g.basis_dim, [&](auto b) {
        constexpr int B = decltype(b)::value;
        const unsigned blocks = blocks_for(r.n_rays * GroupLanes<B>::value);
        if (g.skip)
            grid_taped_kernel<B, true><<<blocks, kGridThreads, 0, s>>>(g, o, r);
        else
            grid_taped_kernel<B, false><<<blocks, kGridThreads, 0, s>>>(g, o, r);
        return hipGetLastError();
    });
}

hipError_t launch_grid_render_bwd(const GridDev& g, const GridRenderOpt& o, const GridRenderBwd& r, hipStream_t s) {
    if (r.n_rays <= 0) return hipSuccess;
    return dispatch_basis(g.basis_dim, [&](auto b) {
        constexpr int B = decltype(b)::value;
        const unsigned blocks = blocks_for(r.n_rays * GroupLanes<B>::value);
        if (g.skip)
            grid_render_bwd_kernel<B, true, false><<<blocks, kGridThreads, 0, s>>>(g, o, r);
        else
            grid_render_bwd_kernel<B, false, false><<<blocks, kGridThreads, 0, s>>>(g, o, r);
        return hipGetLastError();
    });
}

hipError_t launch_grid_sample_bwd(const GridDev& g, const GridSampleBwd& a, hipStream_t s) {
    const int cols = a.want_colors ? 1 + 3 * g.basis_dim : 1;
    if (a.n <= 0) return hipSuccess;
    grid_sample_bwd_kernel<<<blocks_for(a.n * cols), kGridThreads, 0, s>>>(g, a, cols);
    return hipGetLastError();
}

}  // namespace nerf
