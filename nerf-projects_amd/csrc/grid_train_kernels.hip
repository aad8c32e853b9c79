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
// grid_fused_kernel and grid_tv_grad_kernel are written in grid_train_device.h; this file instantiates them without the loss
// terms and without the edge rule, grid_train_losses_kernels.hip with.
#include "grid_train_device.h"

namespace nerf {
namespace {

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
            grid_fused_kernel<B, true, false><<<blocks, kGridThreads, 0, s>>>(g, o, r);
        else
            grid_fused_kernel<B, false, false><<<blocks, kGridThreads, 0, s>>>(g, o, r);
        return hipGetLastError();
    });
}

hipError_t launch_grid_tv_grad(const GridDev& g, const GridTv& a, hipStream_t s) {
    const int64_t n = a.count * (a.end_dim - a.start_dim);
    if (n <= 0) return hipSuccess;
    grid_tv_grad_kernel<false><<<blocks_for(n), kGridThreads, 0, s>>>(g, a);
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
