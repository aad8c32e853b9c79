// Sparse voxel grid training with svox2's regularisers: the instantiations of grid_train_device.h's kernels WITH the beta and
// sparsity terms (grid_fused_kernel, grid_render_bwd_kernel) and WITH the edge rule (grid_tv_grad_kernel). Semantics:
// include/nerf_mi355x.h, "Sparse voxel grid: training with the beta and sparsity losses". Design and measurements: DESIGN.md
// section 7d, addendum.
//
// They are a file of their own so that the instantiations behind nerf_grid_fused_backward, nerf_grid_render_backward and
// nerf_grid_tv_grad (grid_train_kernels.hip, grid_autograd_kernels.hip) stay the code objects they were. Lane layout, marches,
// atomics and mask stores are those kernels'; the terms add, per ray, one exp and one division before the second march and,
// per shaded sample, one addition (beta) and five operations and a division (sparsity) to d_sigma. No LDS, no scratch.
#include "grid_train_device.h"

namespace nerf {

hipError_t launch_grid_fused_losses(const GridDev& g, const GridRenderOpt& o, const GridFused& r, hipStream_t s) {
    if (r.n_rays <= 0) return hipSuccess;
    return dispatch_basis(g.basis_dim, [&](auto b) {
        constexpr int B = decltype(b)::value;
        const unsigned blocks = blocks_for(r.n_rays * GroupLanes<B>::value);
        if (g.skip)
            grid_fused_kernel<B, true, true><<<blocks, kGridThreads, 0, s>>>(g, o, r);
        else
            grid_fused_kernel<B, false, true><<<blocks, kGridThreads, 0, s>>>(g, o, r);
        return hipGetLastError();
    });
}

hipError_t launch_grid_render_bwd_losses(const GridDev& g, const GridRenderOpt& o, const GridRenderBwd& r, hipStream_t s) {
    if (r.n_rays <= 0) return hipSuccess;
    return dispatch_basis(g.basis_dim, [&](auto b) {
        constexpr int B = decltype(b)::value;
        const unsigned blocks = blocks_for(r.n_rays * GroupLanes<B>::value);
        if (g.skip)
            grid_render_bwd_kernel<B, true, true><<<blocks, kGridThreads, 0, s>>>(g, o, r);
        else
            grid_render_bwd_kernel<B, false, true><<<blocks, kGridThreads, 0, s>>>(g, o, r);
        return hipGetLastError();
    });
}

hipError_t launch_grid_tv_grad_edge(const GridDev& g, const GridTv& a, hipStream_t s) {
    const int64_t n = a.count * (a.end_dim - a.start_dim);
    if (n <= 0) return hipSuccess;
    grid_tv_grad_kernel<true><<<blocks_for(n), kGridThreads, 0, s>>>(g, a);
    return hipGetLastError();
}

}  // namespace nerf
