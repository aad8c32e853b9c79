// Sparse voxel grid (Plenoxels) training kernels: the fused render + MSE backward, the total-variation gradient over a range
// of cells, and the masked RMSProp / SGD step. Semantics: include/nerf_mi355x.h, "Sparse voxel grid: training". Design,
// generated-code figures and measurements: DESIGN.md section 7d.
//
// grid_fused_kernel keeps the lane layout of grid_render_kernel (grid_device.h, group_lane): one SH coefficient per lane, a
// ray owns a group of 32 / 16 / 4 lanes at basis_dim 9 / 4 / 1. A ray is marched twice by its group, both times by
// grid_march (grid_device.h). The first march is march_colour, the function grid_render_kernel calls, and leaves the colour
// in registers (channel c in the group's lane c * B); nothing goes through memory between the two. The second march,
// march_colour_bwd, walks the same lattice - the same fp32 additions of t, the same skip data, the same sigma_thresh and
// stop rules - and at every shaded sample scatters the gradients into the 8 corner rows:
// lane (c, k) adds w8 * (weight * Y_k * g_c) to grad_sh[row, c * B + k], so a corner's 12 B * B gradient row is one
// contiguous run of float atomics issued by the group in one instruction, and lanes 0..7 of the group (0..3 twice at
// basis_dim 1) each take one corner's density add and mask byte. The per-sample colour of all three channels, which every
// lane needs for d sigma, is spread with three group-wide shuffles. Control flow is uniform inside a group; groups of a
// wavefront diverge exactly as they do in the renderer.
// Float adds are atomicAdd(float*) = one global_atomic_add_f32 without return (no compare-and-swap loop); the mask is
// written with plain byte stores (every writer stores 1). No LDS, no scratch.
#include "grid_device.h"

namespace nerf {
namespace {

template <int B, bool SKIP>
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
    // second march: the same lattice, gradients scattered
    march_colour_bwd<B, SKIP>(g, opt, rs, gl, yk, gc, remaining, r, gl.busy, true, true);
}

// One thread per (cell of the range, column): svox2's tv_grad_sparse_kernel with ignore_edge = 0, ignore_last_z = 0, no NDC.
// Cell i of the range is node (start + i) mod X Y Z; forward differences to its +x, +y, +z neighbours, an empty or
// out-of-range node counts as 0 and receives nothing.
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
    lk[1] = x + 1 < g.size[0] ? g.links[cell + sx] : -1;
    lk[2] = y + 1 < g.size[1] ? g.links[cell + sy] : -1;
    lk[3] = z + 1 < g.size[2] ? g.links[cell + 1] : -1;
    float v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (!(lk[c] >= 0 && (int64_t)lk[c] < g.capacity)) lk[c] = -1;
        v[c] = lk[c] >= 0 ? a.data[(int64_t)lk[c] * a.cols + col] : 0.0f;
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

// svox2's rmsprop_mask_step_kernel / sgd_mask_step_kernel, one thread per element of the rows whose mask byte is set. Every
// operation is one rounded fp32 operation, in the order written (include/nerf_mi355x.h states it): optim_element of grid_device.h.
template <bool RMSPROP>
__global__ __launch_bounds__(kGridThreads) void grid_optim_step_kernel(GridOptim a) {
    const int64_t tid = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (tid >= a.rows * a.cols) return;
    if (!a.mask[tid / a.cols]) return;
    optim_element<RMSPROP>(a.data, a.rms, tid, a.grad[tid], a.beta, a.lr, a.eps, a.minval);
}

}  // namespace

hipError_t launch_grid_fused(const GridDev& g, const GridRenderOpt& o, const GridFused& r, hipStream_t s) {
    if (r.n_rays <= 0) return hipSuccess;
    return dispatch_basis(g.basis_dim, [&](auto b) {
        constexpr int B = decltype(b)::value;
        const unsigned blocks = blocks_for(r.n_rays * GroupLanes<B>::value);
        if (g.skip)
            grid_fused_kernel<B, true><<<blocks, kGridThreads, 0, s>>>(g, o, r);
        else
            grid_fused_kernel<B, false><<<blocks, kGridThreads, 0, s>>>(g, o, r);
        return hipGetLastError();
    });
}

hipError_t launch_grid_tv_grad(const GridDev& g, const GridTv& a, hipStream_t s) {
    const int64_t n = a.count * (a.end_dim - a.start_dim);
    if (n <= 0) return hipSuccess;
    grid_tv_grad_kernel<<<blocks_for(n), kGridThreads, 0, s>>>(g, a);
    return hipGetLastError();
}

hipError_t launch_grid_optim_step(const GridOptim& a, int rmsprop, hipStream_t s) {
    const int64_t n = a.rows * a.cols;
    if (n <= 0) return hipSuccess;
    if (rmsprop)
        grid_optim_step_kernel<true><<<blocks_for(n), kGridThreads, 0, s>>>(a);
    else
        grid_optim_step_kernel<false><<<blocks_for(n), kGridThreads, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace nerf
