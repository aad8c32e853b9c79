// Sparse voxel grid, palette-quantised colours: the render and sample kernels that read a colour through a node's palette
// index. Semantics: include/nerf_mi355x.h, "Sparse voxel grid: palette-quantised colours". Design and measurements: DESIGN.md 7p.
//
// Tables (grid_internal.h: GridPalette), Q = basis_dim - retain quantised functions, P = 2^bits palette entries:
//   map      uint16 [capacity, Q]       node-major, rows not padded: 18 / 8 / 2 bytes at Q = 9 / 4 / 1
//   colors   half   [Q, P, 3]           the palettes, as the file stores them: an entry's three channels are 6 contiguous bytes
//   retained half   [capacity, retain, 3]
// Why the map is node-major and unpadded. The group of lanes that walks a ray reads, per corner, all Q indices of ONE node, so
// they must lie together (the file's [Q, capacity] would spread them over Q lines). The three lanes (c, k), c = 0, 1, 2, read the
// same two bytes. An 18-byte row straddles a 64-byte line for 8 of every 32 rows (rows are 2-byte aligned, a line holds 3.56 of
// them); padding the row to 32 bytes as 7k pads the half row would end that at 1.78 times the bytes, and bytes are what this
// table exists to save: at 18 bytes a line serves 3.5 nodes' indices, at 32 bytes 2. The padded row was not measured.
//
// Lane mapping: grid_kernels.hip's, one coefficient per lane, groups of 32 / 16 / 4 lanes per ray. Lane (channel c, function k)
//   k <  retain  loads half (k, c) of its node's retained row:                     one load per corner
//   k >= retain  loads index k - retain of its node's map row, then component c of that palette entry: two dependent loads
// and widens the half to fp32 (exact). Everything after that is grid_device.h unchanged - trilerp, shade_channel's shuffle tree
// (restated in ShadePalette, which differs from it in the fetch alone), march_colour - so a render is, bit for bit, the fp32
// kernel's render of the dequantised table. With 0 < retain < basis_dim the two kinds of lane share a group and the fetch
// diverges inside it; the shuffles that follow run converged. No LDS, no scratch, 256-thread workgroups.
#include <algorithm>

#include "grid_fetch_device.h"      // PaletteLane: what lane (c, k) reads of a node

namespace nerf {
namespace {

// shade_channel (grid_device.h) with the fetch above: the same trilerp, the same tree, the same order
template <int B>
struct ShadePalette {
    PaletteLane f;
    __device__ __forceinline__ float operator()(const GridDev&, const int lk[8], const float wa[3], const float wb[3],
                                                const GroupLane& gl, float yk) const {
        float cv[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) cv[c] = lk[c] >= 0 ? f.at(lk[c]) : 0.0f;
        float part = mul(yk, trilerp(cv, wa, wb));
#pragma unroll
        for (int off = 1; off < B; off <<= 1) {
            const float up = __shfl_down(part, off);
            if (gl.k + off < B) part = add(part, up);
        }
        return part;
    }
};

// grid_kernels.hip's grid_render_kernel with that shade
template <int B, bool IMAGE, bool SKIP, bool COUNT>
__global__ __launch_bounds__(kGridThreads) void grid_palette_render_kernel(GridDev g, GridPalette p, GridRenderOpt opt, GridRender r) {
    const GroupLane gl = group_lane<B>();
    if (gl.ray >= r.n_rays) return;
    GridRay rs;
    if (IMAGE)
        camera_ray(r.cam, gl.ray, rs.o, rs.d);
    else
        load_ray(r.origins, r.dirs, gl.ray, rs);
    setup_ray<SKIP>(g, opt, rs);
    const float yk = gl.busy ? sh_basis(gl.k, rs.v[0], rs.v[1], rs.v[2]) : 0.0f;
    const ShadePalette<B> shade{PaletteLane(p, B, gl.col / B, gl.k)};      // (an idle lane reads column 0 and contributes nothing)
    const Colour c = march_colour<B, SKIP, false, COUNT>(g, opt, rs, gl, yk, shade);
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
hipError_t launch_render_b(const GridDev& g, const GridPalette& p, const GridRenderOpt& o, const GridRender& r, hipStream_t s) {
    const unsigned blocks = blocks_for(r.n_rays * GroupLanes<B>::value);
    if (r.counters)
        grid_palette_render_kernel<B, IMAGE, SKIP, true><<<blocks, kGridThreads, 0, s>>>(g, p, o, r);
    else
        grid_palette_render_kernel<B, IMAGE, SKIP, false><<<blocks, kGridThreads, 0, s>>>(g, p, o, r);
    return hipGetLastError();
}

// grid_kernels.hip's grid_sample_kernel: one thread per (point, output column), column 0 = density, 1 + j = SH column j
__global__ __launch_bounds__(kGridThreads) void grid_palette_sample_kernel(GridDev g, GridPalette p, const float* __restrict__ points,
                                                                            int64_t n, int grid_coords, int cols,
                                                                            float* __restrict__ density, float* __restrict__ sh) {
    const int64_t tid = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    const int64_t pt = tid / cols;
    const int j = (int)(tid % cols);
    if (pt >= n) return;
    float x[3], wa[3], wb[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        x[i] = points[pt * 3 + i];
        if (!grid_coords) x[i] = add(g.offset[i], mul(x[i], g.scaling[i]));
    }
    int lk[8];
    load_links(g, point_cell(g, x, wa, wb), lk);
    float cv[8];
    const int B = g.basis_dim;
    const PaletteLane f(p, B, j == 0 ? 0 : (j - 1) / B, j == 0 ? 0 : (j - 1) % B);
#pragma unroll
    for (int c = 0; c < 8; ++c) cv[c] = lk[c] < 0 ? 0.0f : (j == 0 ? g.density[lk[c]] : f.at(lk[c]));
    const float out = trilerp(cv, wa, wb);
    if (j == 0)
        density[pt] = out;
    else
        sh[pt * (3 * B) + (j - 1)] = out;
}

// *out = 1 if any index is >= entries (grid_check_links_kernel's shape)
__global__ __launch_bounds__(kGridThreads) void grid_palette_check_kernel(const uint16_t* __restrict__ map, int64_t n, int entries,
                                                                           int* out) {
    const int64_t stride = (int64_t)gridDim.x * kGridThreads;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * kGridThreads + threadIdx.x; i < n; i += stride) bad = bad || (int)map[i] >= entries;
    if (bad) *out = 1;      // (every writer stores the same value)
}

}  // namespace

hipError_t launch_grid_palette_render(const GridDev& g, const GridPalette& p, const GridRenderOpt& o, const GridRender& r,
                                      hipStream_t s) {
    if (r.n_rays <= 0) return hipSuccess;
    const bool image = r.origins == nullptr, skip = g.skip != nullptr;
    return dispatch_basis(g.basis_dim, [&](auto b) {
        constexpr int B = decltype(b)::value;
        if (image) return skip ? launch_render_b<B, true, true>(g, p, o, r, s) : launch_render_b<B, true, false>(g, p, o, r, s);
        return skip ? launch_render_b<B, false, true>(g, p, o, r, s) : launch_render_b<B, false, false>(g, p, o, r, s);
    });
}

hipError_t launch_grid_palette_sample(const GridDev& g, const GridPalette& p, const float* points, int64_t n, int grid_coords,
                                      int want_colors, float* density, float* sh, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int cols = want_colors ? 1 + 3 * g.basis_dim : 1;
    grid_palette_sample_kernel<<<blocks_for(n * cols), kGridThreads, 0, s>>>(g, p, points, n, grid_coords, cols, density, sh);
    return hipGetLastError();
}

hipError_t launch_grid_palette_check(const uint16_t* map, int64_t n, int entries, int* out, hipStream_t s) {
    hipError_t e = hipMemsetAsync(out, 0, sizeof(int), s);
    if (e != hipSuccess || n <= 0) return e;
    const unsigned blocks = (unsigned)std::min<int64_t>(blocks_for(n), 4096);
    grid_palette_check_kernel<<<blocks, kGridThreads, 0, s>>>(map, n, entries, out);
    return hipGetLastError();
}

}  // namespace nerf
