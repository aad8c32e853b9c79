// Sparse voxel grid, half-precision colours: the SH table packed to fp16 rows, and the render and sample kernels that read
// it. Semantics: include/nerf_mi355x.h, "Sparse voxel grid: half-precision colours". Design and measurements: DESIGN.md 7k.
//
// A packed row (grid_internal.h: grid_half_channel_halfs, grid_half_row_halfs) is channel-major like sh_data, a channel in
// 10 / 4 / 1 slots and the row zero-padded to 32 / 16 / 4 halfs at basis_dim 9 / 4 / 1: 64 / 32 / 8 bytes, so a row lies in
// one 64-byte line, and coefficients (2 j, 2 j + 1) of a channel are one aligned 32-bit word.
//
// A half is widened to fp32 (exact) the moment it is loaded; everything after that is the fp32 arithmetic of grid_device.h -
// grid_march, sample_sigma, trilerp, march_colour - in the same order, so a render is, bit for bit, the fp32 kernel's render of
// the widened table. There is no second march: the kernels below only tell march_colour how a sample is shaded.
//
// Two lane mappings of the render kernel:
//   single  grid_kernels.hip's: one coefficient per lane, shade_channel with a 2-byte load. Groups of 32 / 16 / 4 lanes.
//   pair    lane (channel c, j) loads the word with coefficients (2 j, 2 j + 1) of its channel from each of the 8 corner rows,
//           widens and interpolates both, multiplies by Y_2j and Y_2j+1 and adds the two products: level `off = 1` of
//           shade_channel's tree, whose odd lanes never reach lane 0. The levels 2, 4, 8 of that tree are shuffles at distance
//           1, 2, 4 across the J = 5 / 2 lanes of the channel. A ray owns 16 lanes at basis_dim 9 (15 busy) and 8 at basis_dim 4
//           (6 busy): 4 / 8 rays per wavefront, the same number of load instructions per lane and sample. The busy lane l
//           reads word l of the row. basis_dim 1 has no pairs and renders with `single`.
// As in grid_kernels.hip all control flow is uniform inside a group, no LDS, no scratch, 256-thread workgroups.
#include "grid_fetch_device.h"      // widen

namespace nerf {
namespace {

// ---- pack / unpack ----------------------------------------------------------------------------------------------------------
// one thread per slot of the packed rows (pad slots included: they are written as zero)
__global__ __launch_bounds__(kGridThreads) void grid_pack_half_kernel(GridHalfPack a, int cs, int rh) {
    const int64_t tid = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    const int64_t row = tid / rh;
    const int slot = (int)(tid % rh);
    if (row >= a.rows) return;
    const int c = slot / cs, k = slot % cs, B = a.basis_dim;
    uint16_t out = 0;
    if (c < 3 && k < B) {
        const float x = a.sh[row * (3 * B) + c * B + k];
        const bool over = fabsf(x) > 65504.0f;      // (false for a NaN, which converts to a NaN)
        const float y = over ? copysignf(65504.0f, x) : x;
        out = __builtin_bit_cast(uint16_t, (_Float16)y);      // round to nearest even, subnormals kept
        if (over && a.clamped) atomicAdd(a.clamped, 1ull);
    }
    a.sh_half[(a.row0 + row) * rh + slot] = out;
}

// one thread per fp32 entry
__global__ __launch_bounds__(kGridThreads) void grid_unpack_half_kernel(const uint16_t* __restrict__ sh_half, int64_t rows, int B,
                                                                         int cs, int rh, float* __restrict__ sh) {
    const int64_t tid = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    const int cols = 3 * B;
    const int64_t row = tid / cols;
    const int col = (int)(tid % cols);
    if (row >= rows) return;
    sh[tid] = widen(sh_half[row * rh + (col / B) * cs + col % B]);
}

// ---- sampling: grid_kernels.hip's grid_sample_kernel with the colour columns widened ---------------------------------------------
__global__ __launch_bounds__(kGridThreads) void grid_half_sample_kernel(GridDev g, const float* __restrict__ points, int64_t n,
                                                                         int grid_coords, int cols, int cs, int rh,
                                                                         float* __restrict__ density, float* __restrict__ sh) {
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
    const int B = g.basis_dim;
    const int slot = j == 0 ? 0 : ((j - 1) / B) * cs + (j - 1) % B;
#pragma unroll
    for (int c = 0; c < 8; ++c)
        cv[c] = lk[c] < 0 ? 0.0f : (j == 0 ? g.density[lk[c]] : widen(g.sh_half[(int64_t)lk[c] * rh + slot]));
    const float out = trilerp(cv, wa, wb);
    if (j == 0)
        density[p] = out;
    else
        sh[p * (3 * B) + (j - 1)] = out;
}

// ---- rendering, one coefficient per lane -------------------------------------------------------------------------------------
// shade_channel's fetch: `col` is the lane's slot in the packed row
template <int B>
struct FetchHalf {
    static __device__ __forceinline__ float at(const GridDev& g, int link, int slot) {
        return widen(g.sh_half[(int64_t)link * grid_half_row_halfs(B) + slot]);
    }
};

template <int B>
struct ShadeHalf {
    __device__ __forceinline__ float operator()(const GridDev& g, const int lk[8], const float wa[3], const float wb[3],
                                                const GroupLane& gl, float yk) const {
        return shade_channel<B, FetchHalf<B>>(g, lk, wa, wb, gl.col, gl.k, yk);
    }
};

// ---- rendering, two coefficients per lane ------------------------------------------------------------------------------------
template <int B> struct PairLanes { static constexpr int value = B == 9 ? 16 : 8; };      // lanes of a wavefront that walk one ray

// group_lane for that layout: k is the lane's place j among the J = (B + 1) / 2 lanes of its channel, col the word of the packed
// row it loads (idle lanes read word 0 and contribute nothing)
template <int B>
__device__ __forceinline__ GroupLane group_lane_pair() {
    constexpr int J = (B + 1) / 2;
    const int64_t tid = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    GroupLane gl;
    gl.ray = tid / PairLanes<B>::value;
    gl.lane = (int)(tid % PairLanes<B>::value);
    gl.busy = gl.lane < 3 * J;
    gl.col = gl.busy ? gl.lane : 0;      // channel c starts at word c * grid_half_channel_halfs(B) / 2 = c * J
    gl.k = gl.col % J;
    return gl;
}

template <int B>
struct ShadePair {
    float y1;      // Y_(2j+1); march_colour's yk is Y_2j. Unused where the channel has no coefficient 2 j + 1.
    __device__ __forceinline__ float operator()(const GridDev& g, const int lk[8], const float wa[3], const float wb[3],
                                                const GroupLane& gl, float y0) const {
        constexpr int J = (B + 1) / 2;
        const uint32_t* words = reinterpret_cast<const uint32_t*>(g.sh_half);
        float lo[8], hi[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const uint32_t w = lk[c] >= 0 ? words[(int64_t)lk[c] * (grid_half_row_halfs(B) / 2) + gl.col] : 0u;
            lo[c] = widen((uint16_t)(w & 0xffffu));
            hi[c] = widen((uint16_t)(w >> 16));
        }
        float part = mul(y0, trilerp(lo, wa, wb));
        if (2 * gl.k + 1 < B) part = add(part, mul(y1, trilerp(hi, wa, wb)));      // shade_channel's level off = 1
#pragma unroll
        for (int off = 1; off < J; off <<= 1) {                                      // ... and its levels 2, 4, 8
            const float up = __shfl_down(part, off);
            if (gl.k + off < J) part = add(part, up);
        }
        return part;
    }
};

// grid_kernels.hip's grid_render_kernel on the packed table
template <int B, bool PAIR, bool IMAGE, bool SKIP, bool COUNT>
__global__ __launch_bounds__(kGridThreads) void grid_half_render_kernel(GridDev g, GridRenderOpt opt, GridRender r) {
    constexpr int J = (B + 1) / 2;
    GroupLane gl = PAIR ? group_lane_pair<B>() : group_lane<B>();
    if (gl.ray >= r.n_rays) return;
    GridRay rs;
    if (IMAGE)
        camera_ray(r.cam, gl.ray, rs.o, rs.d);
    else
        load_ray(r.origins, r.dirs, gl.ray, rs);
    setup_ray<SKIP>(g, opt, rs);
    const int channel = gl.col / (PAIR ? J : B);
    Colour c;
    if constexpr (PAIR) {
        const float y0 = gl.busy ? sh_basis(2 * gl.k, rs.v[0], rs.v[1], rs.v[2]) : 0.0f;
        const float y1 = gl.busy && 2 * gl.k + 1 < B ? sh_basis(2 * gl.k + 1, rs.v[0], rs.v[1], rs.v[2]) : 0.0f;
        c = march_colour<B, SKIP, false, COUNT>(g, opt, rs, gl, y0, ShadePair<B>{y1});
    } else {
        const float yk = gl.busy ? sh_basis(gl.k, rs.v[0], rs.v[1], rs.v[2]) : 0.0f;
        gl.col = channel * grid_half_channel_halfs(B) + gl.k;      // from the column of sh_data to the slot of the packed row
        c = march_colour<B, SKIP, false, COUNT>(g, opt, rs, gl, yk, ShadeHalf<B>());
    }
    if (gl.busy && gl.k == 0) r.rgb[gl.ray * 3 + channel] = c.outv;
    if (gl.lane == 0) {
        if (r.log_transmit) r.log_transmit[gl.ray] = c.log_t;
        if (COUNT) {
            atomicAdd(&r.counters[0], (unsigned long long)c.visited);
            atomicAdd(&r.counters[1], (unsigned long long)c.shaded);
        }
    }
}

template <int B, bool PAIR, bool IMAGE, bool SKIP>
hipError_t launch_render_b(const GridDev& g, const GridRenderOpt& o, const GridRender& r, hipStream_t s) {
    const unsigned blocks = blocks_for(r.n_rays * (PAIR ? PairLanes<B>::value : GroupLanes<B>::value));
    if (r.counters)
        grid_half_render_kernel<B, PAIR, IMAGE, SKIP, true><<<blocks, kGridThreads, 0, s>>>(g, o, r);
    else
        grid_half_render_kernel<B, PAIR, IMAGE, SKIP, false><<<blocks, kGridThreads, 0, s>>>(g, o, r);
    return hipGetLastError();
}

template <int B, bool PAIR>
hipError_t launch_render_p(const GridDev& g, const GridRenderOpt& o, const GridRender& r, hipStream_t s) {
    const bool image = r.origins == nullptr, skip = g.skip != nullptr;
    if (image) return skip ? launch_render_b<B, PAIR, true, true>(g, o, r, s) : launch_render_b<B, PAIR, true, false>(g, o, r, s);
    return skip ? launch_render_b<B, PAIR, false, true>(g, o, r, s) : launch_render_b<B, PAIR, false, false>(g, o, r, s);
}

}  // namespace

hipError_t launch_grid_pack_half(const GridHalfPack& a, hipStream_t s) {
    if (a.rows <= 0) return hipSuccess;
    const int rh = grid_half_row_halfs(a.basis_dim);
    grid_pack_half_kernel<<<blocks_for(a.rows * rh), kGridThreads, 0, s>>>(a, grid_half_channel_halfs(a.basis_dim), rh);
    return hipGetLastError();
}

hipError_t launch_grid_unpack_half(const uint16_t* sh_half, int64_t rows, int basis_dim, float* sh, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    grid_unpack_half_kernel<<<blocks_for(rows * 3 * basis_dim), kGridThreads, 0, s>>>(
        sh_half, rows, basis_dim, grid_half_channel_halfs(basis_dim), grid_half_row_halfs(basis_dim), sh);
    return hipGetLastError();
}

hipError_t launch_grid_half_render(const GridDev& g, const GridRenderOpt& o, const GridRender& r, bool pair, hipStream_t s) {
    if (r.n_rays <= 0) return hipSuccess;
    return dispatch_basis(g.basis_dim, [&](auto b) {
        constexpr int B = decltype(b)::value;
        if (B > 1 && pair) return launch_render_p<B, (B > 1)>(g, o, r, s);
        return launch_render_p<B, false>(g, o, r, s);
    });
}

hipError_t launch_grid_half_sample(const GridDev& g, const float* points, int64_t n, int grid_coords, int want_colors,
                                   float* density, float* sh, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int cols = want_colors ? 1 + 3 * g.basis_dim : 1;
    grid_half_sample_kernel<<<blocks_for(n * cols), kGridThreads, 0, s>>>(
        g, points, n, grid_coords, cols, grid_half_channel_halfs(g.basis_dim), grid_half_row_halfs(g.basis_dim), density, sh);
    return hipGetLastError();
}

}  // namespace nerf
