// Sparse voxel grid: training the background layers - the taped background pass, its backward, the total-variation gradient
// of the layers and their masked RMSProp / SGD step. Semantics: include/nerf_mi355x.h, "Sparse voxel grid: background layers,
// training". Design and measurements: DESIGN.md section 7m.
//
// The taped pass and the backward walk the forward's own march, grid_background_device.h: the same set-up, sphere hits,
// texel coordinates, cell, interpolation order, sigma > 0, skip and stop rules (background_march with the forward's 4 x 2
// float4 fetch in the taped pass, background_march_fetch with the group's fetch in the backward), so the taped colour and
// log_transmit are the forward's bits and the backward sees the forward's p, weight and log_T at every shaded step.
// Mapping. The taped pass is the forward's: one lane per ray. The backward gives a ray a group of 32 lanes, lane = (x bit,
// y bit, layer, channel) = one dword of the 4 texels x 2 layers x 4 channels of a step: the group marches its ray together
// (control flow is uniform inside a group; the two groups of a wavefront diverge as two rays do), a lane loads its own dword,
// the interpolation is three xor-shuffles in the forward's order (z, then y, then x: the same lerp on the same operands, so
// v has the forward's bits), every lane forms d_sigma and the three d_col, and adds its own term: a wave-instruction of float
// atomics (atomicAdd(float*) = one global_atomic_add_f32 without return, no compare-and-swap loop) covers 2 rays x 4 texels x
// 32 contiguous bytes instead of 64 lone dwords, and a batch of 5 000 rays fills 2 500 wavefronts instead of 79 (DESIGN.md
// has the A/B against one lane per ray, kept as profiles/microbench/background_bwd_one_lane.patch). The mask is written with
// plain byte stores (every writer stores 1). `remaining` is carried in fp64 as in grid_device.h's march_colour_bwd. No LDS, no
// scratch. Row indices are int64_t: capacity * nlayers * 16 bytes passes 2^31.
#include "grid_background_device.h"

namespace nerf {
namespace {

__global__ __launch_bounds__(kGridThreads) void grid_background_taped_kernel(GridDev g, GridBg bg, GridRenderOpt opt, GridBgTaped r) {
    const int64_t ray = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (ray >= r.n_rays) return;
    GridRay rs;
    load_ray(r.origins, r.dirs, ray, rs);
    float log_t = r.log_transmit[ray];
    double* tb = r.tape_background + ray * 3;
    if (log_t < -25.0f) {      // left alone: no layers, no brightness term, the tape untouched
        tb[0] = tb[1] = tb[2] = 0.0;
        r.log_transmit_out[ray] = log_t;
        return;
    }
    setup_ray<false>(g, opt, rs);
    float* rgb = r.rgb + ray * 3;
    double* tape = r.tape + ray * 3;
    if (!rs.ok) {
        const float b = mul(expf(log_t), opt.background_brightness);
        const double b64 = (double)expf(log_t) * (double)opt.background_brightness;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            rgb[c] = add(rgb[c], b);
            tb[c] = b64;
            tape[c] += b64;
        }
        r.log_transmit_out[ray] = log_t;
        return;
    }
    float out[3] = {0.0f, 0.0f, 0.0f};
    double tot[3] = {0.0, 0.0, 0.0};
    log_t = background_march(g, bg, opt, rs, log_t, [&](const BgSample&, const float4& v, float, float weight, float) {
        const float col[3] = {fmaxf(background_colour(v.x), 0.0f), fmaxf(background_colour(v.y), 0.0f),
                              fmaxf(background_colour(v.z), 0.0f)};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            out[c] = add(out[c], mul(weight, col[c]));
            tot[c] += (double)weight * (double)col[c];      // (a product of two floats is exact in a double)
        }
    });
    const float b = mul(expf(log_t), opt.background_brightness);
    const double b64 = (double)expf(log_t) * (double)opt.background_brightness;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        rgb[c] = add(rgb[c], add(out[c], b));
        tb[c] = tot[c] + b64;
        tape[c] += tot[c] + b64;
    }
    r.log_transmit_out[ray] = log_t;
}

// lanes of a wavefront that walk one ray in the backward: lane = x bit * 16 + y bit * 8 + layer * 4 + channel
constexpr int kBgGroup = 32;

__global__ __launch_bounds__(kGridThreads) void grid_background_bwd_kernel(GridDev g, GridBg bg, GridRenderOpt opt, GridBgBwd r) {
    const int64_t tid = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    const int64_t ray = tid / kBgGroup;
    const int lane = (int)(tid % kBgGroup);
    if (ray >= r.n_rays) return;
    const int ch = lane & 3, layer = (lane >> 2) & 1, ybit = (lane >> 3) & 1, xbit = (lane >> 4) & 1;
    const float log_t0 = r.log_transmit[ray];
    if (log_t0 < -25.0f) return;      // left alone in the forward: no gradient
    GridRay rs;
    load_ray(r.origins, r.dirs, ray, rs);
    setup_ray<false>(g, opt, rs);
    if (!rs.ok) return;               // the brightness term only: no gradient to the layers
    const float gc[3] = {r.grad_rgb[ray * 3 + 0], r.grad_rgb[ray * 3 + 1], r.grad_rgb[ray * 3 + 2]};
    double remaining[3] = {r.tape_background[ray * 3 + 0], r.tape_background[ray * 3 + 1], r.tape_background[ray * 3 + 2]};
    int64_t own = -1;      // this lane's entry of the step: (link * L + l_z + layer) * 4 + ch, or -1 without a row
    background_march_fetch(g, bg, opt, rs, log_t0, [&](const BgSample& s) {
        const int link = background_link(bg, xbit ? s.nx : s.lx, ybit ? s.ny : s.ly);
        own = link < 0 ? -1 : ((int64_t)link * bg.nlayers + s.lz + layer) * 4 + ch;
        const float val = own < 0 ? 0.0f : bg.data[own];
        float other = __shfl_xor(val, 4, kBgGroup);
        const float tz = layer ? lerp1(other, val, s.wz) : lerp1(val, other, s.wz);
        other = __shfl_xor(tz, 8, kBgGroup);
        const float ty = ybit ? lerp1(other, tz, s.wy) : lerp1(tz, other, s.wy);
        other = __shfl_xor(ty, 16, kBgGroup);
        const float tx = xbit ? lerp1(other, ty, s.wx) : lerp1(ty, other, s.wx);
        return make_float4(__shfl(tx, 0, kBgGroup), __shfl(tx, 1, kBgGroup), __shfl(tx, 2, kBgGroup), __shfl(tx, 3, kBgGroup));
    }, [&](const BgSample& s, const float4& v, float dstep, float weight, float log_t) {
        const float col[3] = {background_colour(v.x), background_colour(v.y), background_colour(v.z)};
        float dot = 0.0f;
        double accum64 = 0.0;
        float gv[4];      // d loss / d v_c: the three colours, then sigma
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float colour = fmaxf(col[c], 0.0f);
            dot = add(dot, mul(colour, gc[c]));
            remaining[c] -= (double)weight * (double)colour;
            accum64 += remaining[c] * (double)gc[c];
            gv[c] = col[c] > 0.0f ? mul(mul(0.28209479177387814f, weight), gc[c]) : 0.0f;
        }
        gv[3] = mul(dstep, sub(mul(expf(log_t), dot), (float)accum64));
        if (own < 0) return;
        const float g_own = ch == 0 ? gv[0] : (ch == 1 ? gv[1] : (ch == 2 ? gv[2] : gv[3]));
        const float xo = mul(xbit ? s.wx : sub(1.0f, s.wx), g_own);
        const float val = mul(ybit ? s.wy : sub(1.0f, s.wy), xo);
        const float term = mul(val, layer ? s.wz : sub(1.0f, s.wz));
        if (term != 0.0f) atomicAdd(r.grad_background + own, term);
        if (ch == 0 && r.mask_background) r.mask_background[own >> 2] = 1;
    });
}

// One thread per (cell of the range, channel): svox2's msi_tv_grad_sparse_kernel. Cell i is (start + i) mod (2R R L), z
// fastest; forward differences to (nx, y), (x, ny) - both wrap - and to layer z + 1.
__global__ __launch_bounds__(kGridThreads) void grid_background_tv_kernel(GridBg bg, GridBgTv a) {
    const int64_t tid = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    const int64_t i = tid >> 2;
    if (i >= a.count) return;
    const int ch = (int)(tid & 3);
    const int L = bg.nlayers, R = bg.reso;
    const int64_t cells = (int64_t)2 * R * R * L;
    const int64_t cell = (a.start + i) % cells;
    const int z = (int)(cell % L);
    const int y = (int)((cell / L) % R);
    const int x = (int)(cell / ((int64_t)L * R));
    const int nx = x < 2 * R - 1 ? x + 1 : 0;
    const int ny = y < R - 1 ? y + 1 : 0;
    const int l00 = background_link(bg, x, y), l10 = background_link(bg, nx, y), l01 = background_link(bg, x, ny);
    const int64_t i00 = ((int64_t)l00 * L + z) * 4 + ch, i10 = ((int64_t)l10 * L + z) * 4 + ch, i01 = ((int64_t)l01 * L + z) * 4 + ch;
    const float v00 = l00 >= 0 ? bg.data[i00] : 0.0f;
    const float v10 = l10 >= 0 ? bg.data[i10] : 0.0f;
    const float v01 = l01 >= 0 ? bg.data[i01] : 0.0f;
    const bool has_z = l00 >= 0 && z + 1 < L;
    const float v_nxl = has_z ? bg.data[i00 + 4] : (ch == 3 ? 0.0f : v00);
    float dx = sub(v10, v00), dy = sub(v01, v00), dz = sub(v_nxl, v00);
    const float scale = ch == 3 ? a.scale_sigma : a.scale_color;
    const float idelta = scale / sqrtf(add(add(add(1e-9f, mul(dx, dx)), mul(dy, dy)), mul(dz, dz)));
    dx = mul(dx, (float)(2 * R) * (1.0f / 256.0f));
    dy = mul(dy, (float)R * (1.0f / 256.0f));
    dz = mul(dz, (float)L * (1.0f / 256.0f));
    const float v0 = mul(-add(add(dx, dy), dz), idelta);
    if (l00 >= 0 && v0 != 0.0f) {
        atomicAdd(&a.grad[i00], v0);
        a.mask[i00 >> 2] = 1;
    }
    const float vz = mul(dz, idelta);
    if (has_z && vz != 0.0f) {
        atomicAdd(&a.grad[i00 + 4], vz);
        a.mask[(i00 >> 2) + 1] = 1;
    }
    const float vy = mul(dy, idelta);
    if (l01 >= 0 && vy != 0.0f) {
        atomicAdd(&a.grad[i01], vy);
        a.mask[i01 >> 2] = 1;
    }
    const float vx = mul(dx, idelta);
    if (l10 >= 0 && vx != 0.0f) {
        atomicAdd(&a.grad[i10], vx);
        a.mask[i10 >> 2] = 1;
    }
}

// nerf_grid_optim_step's element (optim_element of grid_device.h) over data [rows, 4] with lr_color for the columns 0..2 and
// lr_sigma for column 3
template <bool RMSPROP>
__global__ __launch_bounds__(kGridThreads) void grid_background_optim_kernel(GridBgOptim a) {
    const int64_t tid = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (tid >= a.rows * 4) return;
    if (!a.mask[tid >> 2]) return;
    optim_element<RMSPROP>(a.data, a.rms, tid, a.grad[tid], a.beta, (tid & 3) == 3 ? a.lr_sigma : a.lr_color, a.eps, a.minval);
}

}  // namespace

hipError_t launch_grid_background_taped(const GridDev& g, const GridBg& bg, const GridRenderOpt& o, const GridBgTaped& r, hipStream_t s) {
    if (r.n_rays <= 0) return hipSuccess;
    grid_background_taped_kernel<<<blocks_for(r.n_rays), kGridThreads, 0, s>>>(g, bg, o, r);
    return hipGetLastError();
}

hipError_t launch_grid_background_bwd(const GridDev& g, const GridBg& bg, const GridRenderOpt& o, const GridBgBwd& r, hipStream_t s) {
    if (r.n_rays <= 0) return hipSuccess;
    grid_background_bwd_kernel<<<blocks_for(r.n_rays * kBgGroup), kGridThreads, 0, s>>>(g, bg, o, r);
    return hipGetLastError();
}

hipError_t launch_grid_background_tv(const GridBg& bg, const GridBgTv& a, hipStream_t s) {
    if (a.count <= 0) return hipSuccess;
    grid_background_tv_kernel<<<blocks_for(a.count * 4), kGridThreads, 0, s>>>(bg, a);
    return hipGetLastError();
}

hipError_t launch_grid_background_optim(const GridBgOptim& a, int rmsprop, hipStream_t s) {
    if (a.rows <= 0) return hipSuccess;
    if (rmsprop)
        grid_background_optim_kernel<true><<<blocks_for(a.rows * 4), kGridThreads, 0, s>>>(a);
    else
        grid_background_optim_kernel<false><<<blocks_for(a.rows * 4), kGridThreads, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace nerf
