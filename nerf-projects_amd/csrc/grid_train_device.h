// Sparse voxel grid training: the kernels that exist in two compile-time variants, without and with svox2's regularisers.
//   grid_fused_kernel<B, SKIP, LOSSES>       the fused render + MSE backward; LOSSES adds the beta and sparsity terms to d_sigma
//   grid_render_bwd_kernel<B, SKIP, LOSSES>  the render backward with a caller's cotangent; LOSSES likewise
//   grid_tv_grad_kernel<EDGE>                the total-variation gradient; EDGE is svox2's ignore_edge
// grid_train_kernels.hip and grid_autograd_kernels.hip instantiate the variants without (the code behind
// nerf_grid_fused_backward, nerf_grid_render_backward and nerf_grid_tv_grad, which it was before the variants existed);
// grid_train_losses_kernels.hip instantiates the variants with. Semantics: include/nerf_mi355x.h, "Sparse voxel grid: training"
// and "Sparse voxel grid: training with the beta and sparsity losses". Design and measurements: DESIGN.md section 7d.
#pragma once
#include "grid_device.h"

namespace nerf {
namespace {

// The lane layout of grid_render_kernel (grid_device.h, group_lane): one SH coefficient per lane, a ray owns a group of
// 32 / 16 / 4 lanes at basis_dim 9 / 4 / 1. A ray is marched twice by its group, both times by grid_march. With LOSSES the
// second march receives the first's final log_transmit from the register it is in (Colour::log_t).
template <int B, bool SKIP, bool LOSSES>
__global__ __launch_bounds__(kGridThreads) void grid_fused_kernel(GridDev g, GridRenderOpt opt, GridFused r) {
    constexpr int GL = GroupLanes<B>::value;
    const GroupLane gl = group_lane<B>();
    if (gl.ray >= r.n_rays) return;
    GridRay rs;
    load_ray(r.origins, r.dirs, gl.ray, rs);
    setup_ray<SKIP>(g, opt, rs);
    const float yk = gl.busy ? sh_basis(gl.k, rs.v[0], rs.v[1], rs.v[2]) : 0.0f;

    // first march: the render, with the tape sum; the colour stays in registers (channel c in the group's lane c * B)
    const Colour c = march_colour<B, SKIP, true, false>(g, opt, rs, gl, yk);
    if (gl.busy && gl.k == 0) r.rgb[gl.ray * 3 + gl.col / B] = c.outv;
    if (gl.lane == 0 && r.log_transmit) r.log_transmit[gl.ray] = c.log_t;
    if (!(rs.ok && rs.tmin <= rs.tmax)) return;      // a miss or a non-finite set-up: nothing to differentiate

    // d loss / d rgb: every lane holds all three channels
    float gc[3];
    double remaining[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float rgb = __shfl(c.outv, ch * B, GL);
        gc[ch] = mul(sub(rgb, r.rgb_gt[gl.ray * 3 + ch]), r.grad_scale);
        remaining[ch] = __shfl(c.tot, ch * B, GL);      // (the background term is part of it)
    }
    // second march: the same lattice, gradients scattered (log_t is the same in every lane of the group)
    march_colour_bwd<B, SKIP, LOSSES>(g, opt, rs, gl, yk, gc, remaining, r, gl.busy, true, true, c.log_t);
}

template <int B, bool SKIP, bool LOSSES>
__global__ __launch_bounds__(kGridThreads) void grid_render_bwd_kernel(GridDev g, GridRenderOpt opt, GridRenderBwd r) {
    const GroupLane gl = group_lane<B>();
    if (gl.ray >= r.n_rays) return;
    GridRay rs;
    load_ray(r.origins, r.dirs, gl.ray, rs);
    setup_ray<SKIP>(g, opt, rs);
    if (!(rs.ok && rs.tmin <= rs.tmax)) return;      // a miss or a non-finite set-up: nothing to differentiate
    const float yk = gl.busy ? sh_basis(gl.k, rs.v[0], rs.v[1], rs.v[2]) : 0.0f;
    float gc[3];
    double remaining[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        gc[c] = r.grad_rgb[gl.ray * 3 + c];
        remaining[c] = r.tape[gl.ray * 3 + c];
    }
    const float log_t_final = LOSSES && r.log_transmit ? r.log_transmit[gl.ray] : 0.0f;
    march_colour_bwd<B, SKIP, LOSSES>(g, opt, rs, gl, yk, gc, remaining, r, gl.busy && r.grad_sh != nullptr,
                                      r.grad_density != nullptr, r.mask != nullptr, log_t_final);
}

// One thread per (cell of the range, column): svox2's tv_grad_sparse_kernel with ignore_edge = EDGE, ignore_last_z = 0, no
// NDC. Cell i of the range is node (start + i) mod X Y Z; forward differences to its +x, +y, +z neighbours. Without EDGE an
// empty or out-of-range node counts as 0 and receives nothing. With EDGE such a neighbour counts as the cell's own value (its
// difference is 0), the cell's own value is still 0 where the cell is empty, and a cell whose own link is exactly row 0 does
// nothing: the reference's literal `*links_ptr == 0`.
template <bool EDGE>
__global__ __launch_bounds__(kGridThreads) void grid_tv_grad_kernel(GridDev g, GridTv a) {
    const int ncol = a.end_dim - a.start_dim;
    const int64_t tid = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    const int64_t i = tid / ncol;
    if (i >= a.count) return;
    const int col = (int)(tid % ncol) + a.start_dim;
    const int64_t n = (int64_t)g.size[0] * g.size[1] * g.size[2];
    const int64_t cell = (a.start + i) % n;
    int x, y, z;
    node_to_xyz(cell, g.size, x, y, z);
    const int sy = g.size[2], sx = g.size[1] * g.size[2];
    int lk[4];      // 000, +x, +y, +z
    lk[0] = g.links[cell];
    if (EDGE && lk[0] == 0) return;
    lk[1] = x + 1 < g.size[0] ? g.links[cell + sx] : -1;
    lk[2] = y + 1 < g.size[1] ? g.links[cell + sy] : -1;
    lk[3] = z + 1 < g.size[2] ? g.links[cell + 1] : -1;
    float v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (!(lk[c] >= 0 && (int64_t)lk[c] < g.capacity)) lk[c] = -1;
        v[c] = lk[c] >= 0 ? a.data[(int64_t)lk[c] * a.cols + col] : (EDGE && c > 0 ? v[0] : 0.0f);
    }
    float dx = sub(v[1], v[0]), dy = sub(v[2], v[0]), dz = sub(v[3], v[0]);
    const float ss = add(add(add(1e-9f, mul(dx, dx)), mul(dy, dy)), mul(dz, dz));
    const float idelta = a.scale / sqrtf(ss);
    dx = mul(dx, a.axis_scale[0]);
    dy = mul(dy, a.axis_scale[1]);
    dz = mul(dz, a.axis_scale[2]);
    const float val[4] = {-add(add(dx, dy), dz), dx, dy, dz};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (lk[c] >= 0 && val[c] != 0.0f) {
            atomicAdd(&a.grad[(int64_t)lk[c] * a.cols + col], mul(val[c], idelta));
            a.mask[lk[c]] = 1;
        }
    }
}

}  // namespace
}  // namespace nerf
