// Sparse voxel grid (Plenoxels) kernels: trilinear ray marching through a grid of densities and spherical-harmonic colour
// coefficients, point sampling, empty-space skip distances, camera rays, and the SH projection of the bake.
// Semantics: include/nerf_mi355x.h, "Sparse voxel grid". Design and measurements: DESIGN.md section 7c.
//
// Mapping of the render kernel: one SH coefficient per lane. A ray owns a GROUP of 32 lanes at basis_dim 9 (27 busy), 16 at
// basis_dim 4 (12 busy), 4 at basis_dim 1 (3 busy): 2, 4 or 16 rays per 64-lane wavefront. Every lane of a group walks the
// same ray and loads the 8 links and 8 densities of a sample redundantly (one address per group: a broadcast in the memory
// pipe); when the sample is shaded, lane c * B + k loads coefficient k of channel c from the 8 corner rows - a corner's
// 12 B * B row is one contiguous read by the group - interpolates it, multiplies by Y_k and the B lanes of a channel are
// summed with __shfl_down inside the group. All control flow is uniform inside a group, so a shuffle only ever reads lanes
// that execute it. Groups of a wavefront diverge (rays end at different t, samples are shaded or not): the lanes of a
// finished or unshaded ray are masked off by EXEC while the other group works. The lane decode (group_lane), the march
// (grid_march) and the colour accumulated along it (march_colour) are grid_device.h's, shared with the taped, fused, depth
// and backward kernels: all of them visit the same samples. No LDS, no scratch, no atomics (except in the
// instrumented launch that counts samples), 256-thread workgroups and few registers so that every SIMD holds its 8 waves:
// the kernel is bound by the dependent link -> row loads, and waves in flight are what hides them.
#include <algorithm>

#include "grid_device.h"

namespace nerf {
namespace {

__global__ __launch_bounds__(kGridThreads) void grid_gen_rays_kernel(GridCam cam, float* __restrict__ origins,
                                                                      float* __restrict__ dirs) {
    const int64_t pix = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (pix >= (int64_t)cam.width * cam.height) return;
    float o[3], d[3];
    camera_ray(cam, pix, o, d);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        origins[pix * 3 + i] = o[i];
        dirs[pix * 3 + i] = d[i];
    }
}

template <int B, bool IMAGE, bool SKIP, bool COUNT>
__global__ __launch_bounds__(kGridThreads) void grid_render_kernel(GridDev g, GridRenderOpt opt, GridRender r) {
    const GroupLane gl = group_lane<B>();
    if (gl.ray >= r.n_rays) return;
    GridRay rs;
    if (IMAGE)
        camera_ray(r.cam, gl.ray, rs.o, rs.d);
    else
        load_ray(r.origins, r.dirs, gl.ray, rs);
    setup_ray<SKIP>(g, opt, rs);
    const float yk = gl.busy ? sh_basis(gl.k, rs.v[0], rs.v[1], rs.v[2]) : 0.0f;
    const Colour c = march_colour<B, SKIP, false, COUNT>(g, opt, rs, gl, yk);
    if (gl.busy && gl.k == 0) r.rgb[gl.ray * 3 + gl.col / B] = c.outv;
    if (gl.lane == 0) {
        if (r.log_transmit) r.log_transmit[gl.ray] = c.log_t;
        if (COUNT) {
            atomicAdd(&r.counters[0], (unsigned long long)c.visited);
            atomicAdd(&r.counters[1], (unsigned long long)c.shaded);
        }
    }
}

template <int B, bool IMAGE, bool SKIP>
hipError_t launch_render_b(const GridDev& g, const GridRenderOpt& o, const GridRender& r, hipStream_t s) {
    const unsigned blocks = blocks_for(r.n_rays * GroupLanes<B>::value);
    if (r.counters)
        grid_render_kernel<B, IMAGE, SKIP, true><<<blocks, kGridThreads, 0, s>>>(g, o, r);
    else
        grid_render_kernel<B, IMAGE, SKIP, false><<<blocks, kGridThreads, 0, s>>>(g, o, r);
    return hipGetLastError();
}

// one thread per (point, output column): column 0 = density, 1 + j = SH column j
__global__ __launch_bounds__(kGridThreads) void grid_sample_kernel(GridDev g, const float* __restrict__ points, int64_t n,
                                                                    int grid_coords, int cols, float* __restrict__ density,
                                                                    float* __restrict__ sh) {
    const int64_t tid = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    const int64_t p = tid / cols;
    const int j = (int)(tid % cols);
    if (p >= n) return;
    float x[3], wa[3], wb[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        x[i] = points[p * 3 + i];
        if (!grid_coords) x[i] = add(g.offset[i], mul(x[i], g.scaling[i]));
    }
    int lk[8];
    load_links(g, point_cell(g, x, wa, wb), lk);
    float cv[8];
    const int row = 3 * g.basis_dim;
#pragma unroll
    for (int c = 0; c < 8; ++c)
        cv[c] = lk[c] < 0 ? 0.0f : (j == 0 ? g.density[lk[c]] : g.sh[(int64_t)lk[c] * row + (j - 1)]);
    const float out = trilerp(cv, wa, wb);
    if (j == 0)
        density[p] = out;
    else
        sh[p * row + (j - 1)] = out;
}

// ---- skip distances ------------------------------------------------------------------------------------
// skip[cell] (indexed by the cell's lowest node): 0 = one of the 8 corners is kept; v >= 1 = every node within v - 1 cells of
// the corners (Chebyshev, clipped to the grid) is empty. Bytes of nodes on the upper faces (no cell) stay 0.
__global__ __launch_bounds__(kGridThreads) void grid_skip_init_kernel(GridDev g, uint8_t* __restrict__ skip) {
    const int64_t n = (int64_t)g.size[0] * g.size[1] * g.size[2];
    const int64_t idx = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (idx >= n) return;
    int ix, jy, kz;
    node_to_xyz(idx, g.size, ix, jy, kz);
    uint8_t v = 0;
    if (ix < g.size[0] - 1 && jy < g.size[1] - 1 && kz < g.size[2] - 1) {
        int lk[8];
        load_links(g, (int)idx, lk);
        bool empty = true;
#pragma unroll
        for (int c = 0; c < 8; ++c) empty = empty && lk[c] < 0;
        v = empty ? 1 : 0;
    }
    skip[idx] = v;
}

// round r: a cell at r whose 26 neighbours (inside the grid) are all >= r becomes r + 1. In place: a neighbour is read
// either before or after its own promotion from r to r + 1, and both values pass the test; smaller values never change.
__global__ __launch_bounds__(kGridThreads) void grid_skip_grow_kernel(GridDev g, uint8_t* skip, int r) {
    const int64_t n = (int64_t)g.size[0] * g.size[1] * g.size[2];
    const int64_t idx = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (idx >= n) return;
    if (skip[idx] != r) return;
    const int sz = g.size[2], sy = g.size[1];
    // (node_to_xyz spelt out on sz, sy: through the function the 31 rounds of accelerate() measured 15 % slower)
    const int kz = (int)(idx % sz), jy = (int)((idx / sz) % sy), ix = (int)(idx / ((int64_t)sz * sy));
    bool all = true;
    for (int a = -1; a <= 1; ++a)
        for (int b = -1; b <= 1; ++b)
            for (int c = -1; c <= 1; ++c) {
                const int x = ix + a, y = jy + b, z = kz + c;
                if (x < 0 || y < 0 || z < 0 || x >= g.size[0] - 1 || y >= sy - 1 || z >= sz - 1) continue;
                all = all && skip[((int64_t)x * sy + y) * sz + z] >= r;
            }
    if (all) skip[idx] = (uint8_t)(r + 1);
}

__global__ __launch_bounds__(kGridThreads) void grid_check_links_kernel(const int32_t* __restrict__ links, int64_t n,
                                                                         int64_t capacity, int* out) {
    const int64_t stride = (int64_t)gridDim.x * kGridThreads;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * kGridThreads + threadIdx.x; i < n; i += stride) bad = bad || (int64_t)links[i] >= capacity;
    if (bad) *out = 1;      // (every writer stores the same value)
}

// ---- the bake's projection: sh_out[row0 + i, c * B + k] = sum_j P[k, j] (sigmoid(raw[i, j, c]) - 0.5) -------------------
constexpr int kProjectMaxP = 4096;
__global__ __launch_bounds__(kGridThreads) void grid_project_sh_kernel(const float* __restrict__ raw, int64_t m, int n_dirs,
                                                                        int B, const float* __restrict__ P,
                                                                        float* __restrict__ sh_out, int64_t row0) {
    __shared__ float sP[kProjectMaxP];
    for (int i = threadIdx.x; i < B * n_dirs; i += kGridThreads) sP[i] = P[i];
    __syncthreads();
    const int cols = 3 * B;
    const int64_t tid = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    const int64_t i = tid / cols;
    const int col = (int)(tid % cols);
    if (i >= m) return;
    const int c = col / B, k = col % B;
    const float* x = raw + i * n_dirs * 4 + c;
    float acc = 0.0f;
    for (int j = 0; j < n_dirs; ++j) {
        const float sg = 1.0f / add(1.0f, expf(-x[j * 4]));
        acc = add(acc, mul(sP[k * n_dirs + j], sub(sg, 0.5f)));
    }
    sh_out[(row0 + i) * cols + col] = acc;
}

}  // namespace

hipError_t launch_grid_render(const GridDev& g, const GridRenderOpt& o, const GridRender& r, hipStream_t s) {
    if (r.n_rays <= 0) return hipSuccess;
    const bool image = r.origins == nullptr, skip = g.skip != nullptr;
    return dispatch_basis(g.basis_dim, [&](auto b) {
        constexpr int B = decltype(b)::value;
        if (image) return skip ? launch_render_b<B, true, true>(g, o, r, s) : launch_render_b<B, true, false>(g, o, r, s);
        return skip ? launch_render_b<B, false, true>(g, o, r, s) : launch_render_b<B, false, false>(g, o, r, s);
    });
}

hipError_t launch_grid_gen_rays(const GridCam& cam, float* origins, float* dirs, hipStream_t s) {
    const int64_t n = (int64_t)cam.width * cam.height;
    if (n <= 0) return hipSuccess;
    grid_gen_rays_kernel<<<blocks_for(n), kGridThreads, 0, s>>>(cam, origins, dirs);
    return hipGetLastError();
}

hipError_t launch_grid_sample(const GridDev& g, const float* points, int64_t n, int grid_coords, int want_colors,
                              float* density, float* sh, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int cols = want_colors ? 1 + 3 * g.basis_dim : 1;
    grid_sample_kernel<<<blocks_for(n * cols), kGridThreads, 0, s>>>(g, points, n, grid_coords, cols, density, sh);
    return hipGetLastError();
}

hipError_t launch_grid_accelerate(const GridDev& g, uint8_t* skip, hipStream_t s) {
    const int64_t n = (int64_t)g.size[0] * g.size[1] * g.size[2];
    grid_skip_init_kernel<<<blocks_for(n), kGridThreads, 0, s>>>(g, skip);
    for (int r = 1; r < kGridSkipCap; ++r) grid_skip_grow_kernel<<<blocks_for(n), kGridThreads, 0, s>>>(g, skip, r);
    return hipGetLastError();
}

hipError_t launch_grid_check_links(const int32_t* links, int64_t n, int64_t capacity, int* out, hipStream_t s) {
    hipError_t e = hipMemsetAsync(out, 0, sizeof(int), s);
    if (e != hipSuccess) return e;
    const unsigned blocks = (unsigned)std::min<int64_t>(blocks_for(n), 4096);
    grid_check_links_kernel<<<blocks, kGridThreads, 0, s>>>(links, n, capacity, out);
    return hipGetLastError();
}

hipError_t launch_grid_project_sh(const float* raw, int64_t m, int n_dirs, int basis_dim, const float* P, float* sh_out,
                                  int64_t row0, hipStream_t s) {
    if (m <= 0) return hipSuccess;
    if (basis_dim * n_dirs > kProjectMaxP) return hipErrorInvalidValue;
    grid_project_sh_kernel<<<blocks_for(m * 3 * basis_dim), kGridThreads, 0, s>>>(raw, m, n_dirs, basis_dim, P, sh_out, row0);
    return hipGetLastError();
}

}  // namespace nerf
