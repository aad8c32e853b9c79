// Sparse voxel grid, the regularisers of the Plenoxels objective as values with exact gradients: total variation of a table
// (svox2's tv() / tv_color()) and the sparsity term of the ray march, each with its backward for autograd. Semantics:
// include/nerf_mi355x.h, "Sparse voxel grid: regularisers as values". Design and measurements: DESIGN.md section 7n.
//
// Total variation: one thread per item (cell, column), the column fastest, so the lanes of a cell share its four link loads
// and read the four table rows as contiguous runs - the mapping of grid_tv_grad_kernel (grid_train_device.h). The value is
// summed without float atomics: a workgroup adds its 256 terms as doubles in LDS in a fixed tree and stores one partial, and
// one workgroup of 1024 threads adds the partials (each thread a consecutive run, then the same tree), divides by the cell
// count and rounds to fp32 once: the order is that of the items, so two calls return the same bits, as the counts of
// compact_device.h do. The backward forms each item's differences and term again and scatters the derivative, times the
// cotangent it reads from device memory, with atomicAdd(float*) = one global_atomic_add_f32 without return.
//
// Sparsity: grid_sparsity_kernel and grid_sparsity_bwd_kernel are written in grid_regularisers_device.h (as the training
// kernels are in grid_train_device.h); this file instantiates them with and without skip data.
#include "grid_regularisers_device.h"

namespace nerf {
namespace {

static_assert(kGridTvValueItems == kGridThreads, "one item per thread, one partial per workgroup");

// Item (cell i of the call, column col): its links (000, +x, +y, +z; anything outside [0, capacity) is -1), the scaled
// differences and the term. false: the item contributes nothing - an entry of `cells` outside the lattice, which is not read
// through, or with `edge` a cell whose own link is exactly row 0.
__device__ __forceinline__ bool tv_item(const GridDev& g, const GridTvValue& a, int64_t i, int col, int lk[4], float d[3],
                                        float& term) {
    const int X = g.size[0], Y = g.size[1], Z = g.size[2];
    int x, y, z;
    int64_t node;
    if (a.cells) {
        node = a.cells_int64 ? ((const int64_t*)a.cells)[i] : (int64_t)((const int32_t*)a.cells)[i];
        if (node < 0 || node >= (int64_t)X * Y * Z) return false;
        node_to_xyz(node, g.size, x, y, z);
    } else {      // cell i of the (X-1)(Y-1)(Z-1) that have all three forward neighbours, z fastest
        z = (int)(i % (Z - 1));
        y = (int)((i / (Z - 1)) % (Y - 1));
        x = (int)(i / ((int64_t)(Z - 1) * (Y - 1)));
        node = ((int64_t)x * Y + y) * Z + z;
    }
    lk[0] = g.links[node];
    if (a.edge && lk[0] == 0) return false;
    lk[1] = x + 1 < X ? g.links[node + (int64_t)Y * Z] : -1;
    lk[2] = y + 1 < Y ? g.links[node + Z] : -1;
    lk[3] = z + 1 < Z ? g.links[node + 1] : -1;
    float v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (!(lk[c] >= 0 && (int64_t)lk[c] < g.capacity)) lk[c] = -1;
        v[c] = lk[c] >= 0 ? a.data[(int64_t)lk[c] * a.cols + col] : (a.edge && c > 0 ? v[0] : 0.0f);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = mul(sub(v[k + 1], v[0]), a.axis_scale[k]);
    term = sqrtf(add(add(add(1e-5f, mul(d[0], d[0])), mul(d[1], d[1])), mul(d[2], d[2])));
    return true;
}

// part[0] = the sum of the N doubles in part, added in a fixed tree (N a power of two = the workgroup's threads)
template <int N>
__device__ __forceinline__ void tree_sum(double* part) {
    __syncthreads();
    for (int s = N / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
}

__global__ __launch_bounds__(kGridThreads) void grid_tv_value_kernel(GridDev g, GridTvValue a) {
    __shared__ double part[kGridThreads];
    const int ncol = a.end_dim - a.start_dim;
    const int64_t tid = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    const int64_t i = tid / ncol;
    double t = 0.0;
    if (i < a.count) {
        int lk[4];
        float d[3], term;
        if (tv_item(g, a, i, (int)(tid % ncol) + a.start_dim, lk, d, term)) t = (double)term;
    }
    part[threadIdx.x] = t;
    tree_sum<kGridThreads>(part);
    if (threadIdx.x == 0) a.partials[blockIdx.x] = part[0];
}

// one workgroup: thread t adds the `per` consecutive partials from t * per, then the tree; n = 0 stores 0
__global__ __launch_bounds__(1024) void grid_tv_value_finish_kernel(const double* partials, int64_t n, int64_t count, float* value) {
    __shared__ double part[1024];
    const int64_t t = threadIdx.x;
    const int64_t per = (n + 1023) / 1024;
    const int64_t lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    double sum = 0.0;
    for (int64_t k = lo; k < hi; ++k) sum += partials[k];
    part[t] = sum;
    tree_sum<1024>(part);
    if (t == 0) *value = count > 0 ? (float)(part[0] / (double)count) : 0.0f;
}

__global__ __launch_bounds__(kGridThreads) void grid_tv_value_bwd_kernel(GridDev g, GridTvValue a) {
    const int ncol = a.end_dim - a.start_dim;
    const int64_t tid = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    const int64_t i = tid / ncol;
    if (i >= a.count) return;
    const int col = (int)(tid % ncol) + a.start_dim;
    int lk[4];
    float d[3], term;
    if (!tv_item(g, a, i, col, lk, d, term)) return;
    const float w = a.grad_value[0] / (float)a.count;
    const float sd[3] = {mul(a.axis_scale[0], d[0]), mul(a.axis_scale[1], d[1]), mul(a.axis_scale[2], d[2])};
    const float q[4] = {-add(add(sd[0], sd[1]), sd[2]) / term, sd[0] / term, sd[1] / term, sd[2] / term};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (lk[c] < 0) continue;
        const float v = mul(w, q[c]);
        if (v != 0.0f) atomicAdd(&a.grad[(int64_t)lk[c] * a.cols + col], v);
    }
}

}  // namespace

hipError_t launch_grid_tv_value(const GridDev& g, const GridTvValue& a, hipStream_t s) {
    const int64_t items = a.count * (a.end_dim - a.start_dim);
    const int64_t blocks = items > 0 ? (items + kGridThreads - 1) / kGridThreads : 0;
    if (blocks > 0) {
        grid_tv_value_kernel<<<(unsigned)blocks, kGridThreads, 0, s>>>(g, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    grid_tv_value_finish_kernel<<<1, 1024, 0, s>>>(a.partials, blocks, a.count, a.value);
    return hipGetLastError();
}

hipError_t launch_grid_tv_value_bwd(const GridDev& g, const GridTvValue& a, hipStream_t s) {
    const int64_t items = a.count * (a.end_dim - a.start_dim);
    if (items <= 0) return hipSuccess;
    grid_tv_value_bwd_kernel<<<blocks_for(items), kGridThreads, 0, s>>>(g, a);
    return hipGetLastError();
}

hipError_t launch_grid_sparsity(const GridDev& g, const GridRenderOpt& o, const GridSparsity& r, hipStream_t s) {
    if (r.n_rays <= 0) return hipSuccess;
    if (g.skip)
        grid_sparsity_kernel<true><<<blocks_for(r.n_rays), kGridThreads, 0, s>>>(g, o, r);
    else
        grid_sparsity_kernel<false><<<blocks_for(r.n_rays), kGridThreads, 0, s>>>(g, o, r);
    return hipGetLastError();
}

hipError_t launch_grid_sparsity_bwd(const GridDev& g, const GridRenderOpt& o, const GridSparsity& r, hipStream_t s) {
    if (r.n_rays <= 0) return hipSuccess;
    if (g.skip)
        grid_sparsity_bwd_kernel<true><<<blocks_for(r.n_rays), kGridThreads, 0, s>>>(g, o, r);
    else
        grid_sparsity_bwd_kernel<false><<<blocks_for(r.n_rays), kGridThreads, 0, s>>>(g, o, r);
    return hipGetLastError();
}

}  // namespace nerf
