// Sparse voxel grid: the device functions the grid kernels (rendering, training, resampling, components) share, so that all
// walk the same sample lattice with the same fp32 operations: rounded arithmetic, the SH basis, the trilinear set-up, the ray
// set-up, the one march (grid_march: the stall rule, the cell, the skip rule, the links, the density) and, on it, the colour
// march forward (march_colour) and backward (march_colour_bwd). Semantics: include/nerf_mi355x.h, "Sparse voxel grid".
#pragma once
#include <type_traits>

#include "grid_internal.h"

namespace nerf {
namespace {

constexpr int kGridThreads = 256;

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kGridThreads - 1) / kGridThreads); }      // one thread per item

// f(std::integral_constant<int, B>) for the basis_dim B the kernels are built for
template <class F>
hipError_t dispatch_basis(int basis_dim, F&& f) {
    switch (basis_dim) {
        case 9: return f(std::integral_constant<int, 9>());
        case 4: return f(std::integral_constant<int, 4>());
        case 1: return f(std::integral_constant<int, 1>());
    }
    return hipErrorInvalidValue;
}

// flat C-order index of a node (z fastest) -> its coordinates
__device__ __forceinline__ void node_to_xyz(int64_t idx, const int32_t size[3], int& ix, int& iy, int& iz) {
    iz = (int)(idx % size[2]);
    iy = (int)((idx / size[2]) % size[1]);
    ix = (int)(idx / ((int64_t)size[2] * size[1]));
}

__device__ __forceinline__ float mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float sub(float a, float b) { return __fsub_rn(a, b); }

// lanes of a wavefront that walk one ray: one SH coefficient per lane
template <int B> struct GroupLanes { static constexpr int value = B == 9 ? 32 : (B == 4 ? 16 : 4); };

// this thread in that layout; a whole group has the same ray (and leaves together where ray >= n_rays)
struct GroupLane {
    int64_t ray;
    int lane;      // of the group
    bool busy;     // lane < 3 B: it owns coefficient k of channel col / B
    int col, k;    // idle lanes of a group read column 0 and contribute nothing
};
template <int B>
__device__ __forceinline__ GroupLane group_lane() {
    const int64_t tid = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    GroupLane gl;
    gl.ray = tid / GroupLanes<B>::value;
    gl.lane = (int)(tid % GroupLanes<B>::value);
    gl.busy = gl.lane < 3 * B;
    gl.col = gl.busy ? gl.lane : 0;
    gl.k = gl.col % B;
    return gl;
}

// svox2 utils.eval_sh_bases, fp32, the reference's operation order
__device__ __forceinline__ float sh_basis(int k, float x, float y, float z) {
    switch (k) {
        case 0: return 0.28209479177387814f;
        case 1: return mul(-0.4886025119029199f, y);
        case 2: return mul(0.4886025119029199f, z);
        case 3: return mul(-0.4886025119029199f, x);
        case 4: return mul(1.0925484305920792f, mul(x, y));
        case 5: return mul(-1.0925484305920792f, mul(y, z));
        case 6: return mul(0.31539156525252005f, sub(sub(mul(2.0f, mul(z, z)), mul(x, x)), mul(y, y)));
        case 7: return mul(-1.0925484305920792f, mul(x, z));
        default: return mul(0.5462742152960396f, sub(mul(x, x), mul(y, y)));
    }
}

// base cell and weights of a position in grid coordinates (clamped to the node range): the reference's trilerp set-up
__device__ __forceinline__ void cell_of(float p, int size, int& l, float& wb) {
    p = fminf(fmaxf(p, 0.0f), (float)(size - 1));
    l = min((int)p, size - 2);
    wb = sub(p, (float)l);
}

// z, then y, then x; wa = 1 - wb (svox2.py:748-755)
__device__ __forceinline__ float trilerp(const float v[8], const float wa[3], const float wb[3]) {
    const float c00 = add(mul(v[0], wa[2]), mul(v[1], wb[2]));
    const float c01 = add(mul(v[2], wa[2]), mul(v[3], wb[2]));
    const float c10 = add(mul(v[4], wa[2]), mul(v[5], wb[2]));
    const float c11 = add(mul(v[6], wa[2]), mul(v[7], wb[2]));
    const float c0 = add(mul(c00, wa[1]), mul(c01, wb[1]));
    const float c1 = add(mul(c10, wa[1]), mul(c11, wb[1]));
    return add(mul(c0, wa[0]), mul(c1, wb[0]));
}

// base cell (returned: its index into links / skip) and trilinear weights of a point in grid coordinates
__device__ __forceinline__ int point_cell(const GridDev& g, const float x[3], float wa[3], float wb[3]) {
    int l[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        cell_of(x[i], g.size[i], l[i], wb[i]);
        wa[i] = sub(1.0f, wb[i]);
    }
    return (l[0] * g.size[1] + l[1]) * g.size[2] + l[2];
}

// weight of corner c (x, y, z bits) = (wx * wy) * wz, in that order
__device__ __forceinline__ float corner_weight(int c, const float wa[3], const float wb[3]) {
    return mul(mul((c & 4) ? wb[0] : wa[0], (c & 2) ? wb[1] : wa[1]), (c & 1) ? wb[2] : wa[2]);
}

// the 8 links of base cell `base` (corner order 000, 001, 010, ..., 111 = x, y, z bits); anything outside [0, capacity) is -1
__device__ __forceinline__ void load_links(const GridDev& g, int base, int lk[8]) {
    const int sy = g.size[2], sx = g.size[1] * g.size[2];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int v = g.links[base + ((c >> 2) & 1) * sx + ((c >> 1) & 1) * sy + (c & 1)];
        lk[c] = (v >= 0 && (int64_t)v < g.capacity) ? v : -1;
    }
}

// The NDC warp of forward-facing scenes: svox2.utils.convert_to_ndc with near = 1, then the normalisation of its two callers
// (Camera.gen_rays, LLFFDataset.gen_rays). fp32, every operation rounded on its own and in the reference's order, so that
// hipcc contracts nothing:
//     t  = (1 - oz) / dz
//     o += t * d                                   (a product and a sum, not an fma)
//     o' = (cx * (ox / oz),  cy * (oy / oz),  1 - 2 / oz)
//     d' = (cx * (dx / dz - ox / oz),  cy * (dy / dz - oy / oz),  2 / oz)
//     n  = sqrt(fma(d'z, d'z, fma(d'y, d'y, d'x * d'x)))         (torch.norm's vectorised CPU sum of squares)
//     d' = d' / n
// Non-finite results (dz == 0, oz == 0) are passed on: setup_ray makes such a ray a miss.
__device__ __forceinline__ void rays_to_ndc(float coeffx, float coeffy, float o[3], float d[3]) {
    const float t = __fdiv_rn(sub(1.0f, o[2]), d[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = add(o[i], mul(t, d[i]));
    const float ox = __fdiv_rn(o[0], o[2]), oy = __fdiv_rn(o[1], o[2]), two_oz = __fdiv_rn(2.0f, o[2]);
    const float dx = mul(coeffx, sub(__fdiv_rn(d[0], d[2]), ox));
    const float dy = mul(coeffy, sub(__fdiv_rn(d[1], d[2]), oy));
    // sqrtf: the correctly rounded root (hipcc's default)
    const float n = sqrtf(__fmaf_rn(two_oz, two_oz, __fmaf_rn(dy, dy, mul(dx, dx))));
    o[0] = mul(coeffx, ox);
    o[1] = mul(coeffy, oy);
    o[2] = sub(1.0f, two_oz);
    d[0] = __fdiv_rn(dx, n);
    d[1] = __fdiv_rn(dy, n);
    d[2] = __fdiv_rn(two_oz, n);
}

// svox2 Camera.gen_rays: fp64, rounded to fp32 at the end; then, for an NDC camera (c.ndc[0] > 0, the same for every lane),
// rays_to_ndc on the rounded ray, as svox2's Python does
__device__ __forceinline__ void camera_ray(const GridCam& c, int64_t pix, float o[3], float d[3]) {
    const int py = (int)(pix / c.width), px = (int)(pix % c.width);
    double xx = ((double)px + 0.5 - c.cx) / c.fx;
    double yy = ((double)py + 0.5 - c.cy) / c.fy;
    double zz = 1.0;
    const double n = sqrt(xx * xx + yy * yy + zz * zz);
    xx /= n;
    yy /= n;
    zz /= n;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        d[i] = (float)(c.c2w[i * 4 + 0] * xx + c.c2w[i * 4 + 1] * yy + c.c2w[i * 4 + 2] * zz);
        o[i] = (float)c.c2w[i * 4 + 3];
    }
    if (c.ndc[0] > 0.0f) rays_to_ndc(c.ndc[0], c.ndc[1], o, d);
}

// ---- ray set-up (svox2.py:662-693) ----
struct GridRay {
    float o[3], d[3];      // origin and unit direction in grid coordinates
    float v[3];            // unit world direction (the SH argument)
    float delta_scale, tmin, tmax;
    bool ok;               // the set-up is finite: the ray is marched (if tmin <= tmax)
    bool skip_ok;          // skip data may be used (positions exact to 1/16)
};

__device__ __forceinline__ void load_ray(const float* origins, const float* dirs, int64_t ray, GridRay& rs) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        rs.o[i] = origins[ray * 3 + i];
        rs.d[i] = dirs[ray * 3 + i];
    }
}

// in: r.o, r.d = world origin and direction (need not be unit)
template <bool SKIP>
__device__ __forceinline__ void setup_ray(const GridDev& g, const GridRenderOpt& opt, GridRay& r) {
    float* o = r.o;
    float* d = r.d;
    float* v = r.v;
    const float dn = sqrtf(add(add(mul(d[0], d[0]), mul(d[1], d[1])), mul(d[2], d[2])));
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        o[i] = add(g.offset[i], mul(o[i], g.scaling[i]));
        v[i] = d[i] / dn;
        d[i] = mul(v[i], g.scaling[i]);
    }
    const float delta_scale = 1.0f / sqrtf(add(add(mul(d[0], d[0]), mul(d[1], d[1])), mul(d[2], d[2])));
    float tmin = -1e9f, tmax = 1e9f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        d[i] = mul(d[i], delta_scale);
        const float inv = 1.0f / d[i];
        const float t1 = mul(sub(-0.5f, o[i]), inv);
        const float t2 = mul(sub((float)g.size[i] - 0.5f, o[i]), inv);
        const bool flat = d[i] == 0.0f;
        tmin = fmaxf(tmin, flat ? -1e9f : fminf(t1, t2));
        tmax = fminf(tmax, flat ? 1e9f : fmaxf(t1, t2));
    }
    tmin = fmaxf(tmin, opt.near_clip);
    // A ray is marched only if its set-up is finite: a zero, NaN or infinite direction or origin is a miss (background,
    // log_transmit 0), whatever fminf / fmaxf made of the NaNs above.
    bool ok = dn > 0.0f && isfinite(dn) && isfinite(delta_scale) && isfinite(tmin) && isfinite(tmax);
    float reach_o = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        ok = ok && isfinite(o[i]) && isfinite(d[i]);
        reach_o = fmaxf(reach_o, fabsf(o[i]));
    }
    r.delta_scale = delta_scale;
    r.tmin = tmin;
    r.tmax = tmax;
    r.ok = ok;
    // the skip proof (header) needs positions exact to 1/16: |o|, |t| < 2^17 grid units; farther rays march plainly
    r.skip_ok = SKIP && reach_o < kGridSkipMaxT && fabsf(tmin) < kGridSkipMaxT && fabsf(tmax) < kGridSkipMaxT;
}

// the sample at t: its point_cell
__device__ __forceinline__ int march_cell(const GridDev& g, const GridRay& r, float t, float wa[3], float wb[3]) {
    const float x[3] = {add(r.o[0], mul(t, r.d[0])), add(r.o[1], mul(t, r.d[1])), add(r.o[2], mul(t, r.d[2]))};
    return point_cell(g, x, wa, wb);
}

// The skip rule at a sample t0 in a cell of skip value sv > 0: every node within sv - 1 cells of this cell's corners is
// empty, so are this sample and every later one whose t (the accumulated value itself, no estimate of it) is within
// sv - 1 - 1/16 of this one's. Returns the t of the next sample to look at; t_next = t0 + step_size.
__device__ __forceinline__ float skip_jump(float t0, float t_next, int sv, float step_size) {
    const float reach = (float)(sv - 1) - 0.0625f;
    float t = t_next;
    while (sub(t, t0) <= reach) {
        const float tn = add(t, step_size);
        if (!(tn > t)) break;
        t = tn;
    }
    return t;
}

// the densities at the 8 links (an empty corner is 0) interpolated
__device__ __forceinline__ float sample_sigma(const GridDev& g, const int lk[8], const float wa[3], const float wb[3]) {
    float cv[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) cv[c] = lk[c] >= 0 ? g.density[lk[c]] : 0.0f;
    return trilerp(cv, wa, wb);
}

// how shade_channel fetches column `col` of row `link`: here from the fp32 table; grid_half_kernels.hip widens a packed half
template <int B>
struct FetchFloat {
    static __device__ __forceinline__ float at(const GridDev& g, int link, int col) { return g.sh[(int64_t)link * (3 * B) + col]; }
};

// lane (channel c, coefficient k = col % B): Y_k times the interpolated coefficient, summed over the B lanes of the channel;
// the sum is complete in the lane with k == 0
template <int B, class Fetch = FetchFloat<B>>
__device__ __forceinline__ float shade_channel(const GridDev& g, const int lk[8], const float wa[3], const float wb[3], int col,
                                               int k, float yk) {
    float cv[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) cv[c] = lk[c] >= 0 ? Fetch::at(g, lk[c], col) : 0.0f;
    float part = mul(yk, trilerp(cv, wa, wb));
#pragma unroll
    for (int off = 1; off < B; off <<= 1) {
        const float up = __shfl_down(part, off);
        if (k + off < B) part = add(part, up);
    }
    return part;
}

// how march_colour shades a sample: a callable (g, lk, wa, wb, gl, yk) -> the channel's sum, complete in the lanes with k == 0.
// This one is shade_channel on the fp32 table; the half-precision kernels pass their own.
template <int B>
struct ShadeFloat {
    __device__ __forceinline__ float operator()(const GridDev& g, const int lk[8], const float wa[3], const float wb[3],
                                                const GroupLane& gl, float yk) const {
        return shade_channel<B>(g, lk, wa, wb, gl.col, gl.k, yk);
    }
};

// ---- the one march --------------------------------------------------------------------------------------------------------
// Every kernel that walks a ray walks it here, so all of them visit the same samples, bit for bit. For a ray that is marched
// (rs.ok && rs.tmin <= rs.tmax): at(t, lk, wa, wb, sigma) is called at every sample whose links are loaded - every sample
// the skip rule does not pass over - in march order. The callback applies its own density threshold and returns true where
// the ray ends. The first sample needs no test against tmax (the precondition is that test), so the loop tests at its end:
// written with the test at its head, the same march cost the plain render 2 % (profiles/grid_march_ab.md).
template <bool SKIP, class F>
__device__ __forceinline__ void grid_march(const GridDev& g, const GridRenderOpt& opt, const GridRay& rs, F&& at) {
    float t = rs.tmin;
    do {
        // the march ends unconditionally: every pass through this loop advances t by at least one addition of step_size,
        // and a ray whose t no longer changes under that addition (t so large that step_size is below half an ulp) is left
        // at once
        const float t_next = add(t, opt.step_size);
        if (!(t_next > t)) break;
        float wa[3], wb[3];
        const int base = march_cell(g, rs, t, wa, wb);
        if (SKIP) {
            const int sv = rs.skip_ok ? g.skip[base] : 0;
            if (sv > 0) {
                t = skip_jump(t, t_next, sv, opt.step_size);
                continue;
            }
        }
        int lk[8];
        load_links(g, base, lk);
        if (at(t, lk, wa, wb, sample_sigma(g, lk, wa, wb))) break;
        t = t_next;
    } while (t <= rs.tmax);
}

// ---- the colour march, forward --------------------------------------------------------------------------------------------
// what lane (channel, coefficient) of a ray's group holds after it; outv and tot are complete in the lanes with k == 0
struct Colour {
    float outv = 0.0f, log_t = 0.0f;      // the channel with its background term; log_transmit (-1e3 where the ray stopped)
    double tot = 0.0;                      // TAPE: the channel once more, as the fp64 sum of its exact terms
    // COUNT: samples whose links were loaded / that were shaded. 32 bits hold a ray's: t advances only while step_size is
    // above half an ulp of t, |t| < 2^24 step_size, by at least half a step_size per sample: fewer than 2^26 samples
    unsigned visited = 0, shaded = 0;
};

// grid_render_kernel, grid_taped_kernel and the first march of grid_fused_kernel: at every sample above sigma_thresh the
// channel is shaded, weighted and accumulated, and the ray stops below stop_thresh. A ray that is not marched is background.
template <int B, bool SKIP, bool TAPE, bool COUNT, class Shade = ShadeFloat<B>>
__device__ __forceinline__ Colour march_colour(const GridDev& g, const GridRenderOpt& opt, const GridRay& rs, const GroupLane& gl,
                                               float yk, const Shade& shade = Shade()) {
    Colour c;
    if (rs.ok && rs.tmin <= rs.tmax) {
        const float neg_step = -opt.step_size;
        grid_march<SKIP>(g, opt, rs, [&](float, const int* lk, const float* wa, const float* wb, float sigma) {
            if (COUNT) ++c.visited;
            if (!(sigma > opt.sigma_thresh)) return false;
            if (COUNT) ++c.shaded;
            const float part = shade(g, lk, wa, wb, gl, yk);
            const float a = mul(mul(neg_step, sigma), rs.delta_scale);
            const float weight = mul(expf(c.log_t), sub(1.0f, expf(a)));
            const float colour = fmaxf(add(part, 0.5f), 0.0f);
            c.outv = add(c.outv, mul(weight, colour));
            if (TAPE) c.tot += (double)weight * (double)colour;      // (a product of two floats is exact in a double)
            c.log_t = add(c.log_t, a);
            if (expf(c.log_t) < opt.stop_thresh) {
                c.log_t = -1e3f;
                return true;
            }
            return false;
        });
    }
    c.outv = add(c.outv, mul(expf(c.log_t), opt.background_brightness));
    if (TAPE) c.tot += (double)expf(c.log_t) * (double)opt.background_brightness;
    return c;
}

// ---- the colour march, backward -------------------------------------------------------------------------------------------
// grid_render_bwd_kernel and the second march of grid_fused_kernel, for a ray that is marched: the same lattice, and at every
// shaded sample the gradients are scattered into the 8 corner rows. gc[c] = d loss / d rgb[c]. r.grad_sh, r.grad_density and
// r.mask are written where want_sh (false in idle lanes), want_density and want_mask say so.
// remaining[c] = what the samples not yet passed, and the background, still add to channel c; it starts as the forward's
// `tot`. It is the one quantity of the backward that is a difference of large, nearly equal sums (the colour minus what the
// passed samples gave); in fp32 its rounding, 6e-8 of the whole colour, is a relative 1e-3 of the small density gradients
// behind a bright sample, which RMSProp's g / (sqrt(rms) + eps) turns into density errors of 1e-3. Kept in fp64, built from
// and reduced by the very same exact products, it is exact to 1e-16 of the colour; everything else is fp32.
// LOSSES (include/nerf_mi355x.h, "Sparse voxel grid: training with the beta and sparsity losses"): svox2's two regularisers
// folded into d_sigma, from r.beta_loss, r.sparsity_loss and the forward's final log_transmit of this ray, log_t_final. A
// compile-time variant: without it this is the code it was before the terms existed, and nothing of them is read.
template <int B, bool SKIP, bool LOSSES = false, class R>
__device__ __forceinline__ void march_colour_bwd(const GridDev& g, const GridRenderOpt& opt, const GridRay& rs, const GroupLane& gl,
                                                 float yk, const float gc[3], double remaining[3], const R& r, bool want_sh,
                                                 bool want_density, bool want_mask, float log_t_final = 0.0f) {
    constexpr int GL = GroupLanes<B>::value;
    constexpr int DL = GL < 8 ? GL : 8;      // lanes of a group that share the 8 density adds
    const float g_own = gl.col / B == 0 ? gc[0] : (gl.col / B == 1 ? gc[1] : gc[2]);
    const float step_ds = mul(opt.step_size, rs.delta_scale);
    const float neg_step = -opt.step_size;
    float log_t = 0.0f;
    float c_beta = 0.0f;      // d (beta term) / d log_T of the whole ray: the same at every sample
    if (LOSSES && r.beta_loss > 0.0f) {
        const float t_in = expf(log_t_final);
        c_beta = mul(r.beta_loss, sub(1.0f, __fdiv_rn(t_in, add(sub(1.0f, t_in), 1e-3f))));
    }
    grid_march<SKIP>(g, opt, rs, [&](float, const int* lk, const float* wa, const float* wb, float sigma) {
        if (!(sigma > opt.sigma_thresh)) return false;
        // (formed here, while few values are live: at the end of the sample it costs a wave of occupancy at basis_dim 4)
        float d_sparsity = 0.0f;
        if (LOSSES && r.sparsity_loss > 0.0f)
            d_sparsity = mul(r.sparsity_loss, __fdiv_rn(mul(4.0f, sigma), add(1.0f, mul(2.0f, mul(sigma, sigma)))));
        const float part = shade_channel<B>(g, lk, wa, wb, gl.col, gl.k, yk);
        const float raw = add(part, 0.5f);      // complete in the lanes with k == 0
        const float a = mul(mul(neg_step, sigma), rs.delta_scale);
        const float weight = mul(expf(log_t), sub(1.0f, expf(a)));
        log_t = add(log_t, a);
        float dot = 0.0f, raw_own = 0.0f;
        double accum64 = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float rc = __shfl(raw, c * B, GL);
            const float colour = fmaxf(rc, 0.0f);
            dot = add(dot, mul(colour, gc[c]));
            remaining[c] -= (double)weight * (double)colour;
            accum64 += remaining[c] * (double)gc[c];
            if (gl.col / B == c) raw_own = rc;
        }
        float accum = (float)accum64;
        if (LOSSES && r.beta_loss > 0.0f) accum = add(accum, c_beta);
        float d_sigma = mul(step_ds, sub(mul(expf(log_t), dot), accum));
        if (LOSSES && r.sparsity_loss > 0.0f) d_sigma = add(d_sigma, d_sparsity);
        // max(0, .) passes the gradient where its argument is >= 0 (torch.clamp_min)
        const float d_coef = raw_own >= 0.0f ? mul(mul(weight, yk), g_own) : 0.0f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            if (lk[c] < 0) continue;
            const float w8 = corner_weight(c, wa, wb);
            if (want_sh) {
                const float v = mul(w8, d_coef);
                if (v != 0.0f) atomicAdd(&r.grad_sh[(int64_t)lk[c] * (3 * B) + gl.col], v);
            }
            if (gl.lane == c % DL) {
                if (want_density) atomicAdd(&r.grad_density[lk[c]], mul(w8, d_sigma));
                if (want_mask) r.mask[lk[c]] = 1;
            }
        }
        return expf(log_t) < opt.stop_thresh;
    });
}

// One element of svox2's rmsprop_mask_step_kernel / sgd_mask_step_kernel (include/nerf_mi355x.h, nerf_grid_optim_step): every
// operation one rounded fp32 operation, in the order written; fmaxf drops a NaN, so a NaN update lands on minval. Shared by the
// foreground's and the background's step kernels.
template <bool RMSPROP>
__device__ __forceinline__ void optim_element(float* data, float* rms, int64_t i, float gr, float beta, float lr, float eps,
                                              float minval) {
    if (RMSPROP) {
        const float g2 = mul(gr, gr);
        float r = rms[i];
        r = r == 0.0f ? g2 : add(g2, mul(beta, sub(r, g2)));
        rms[i] = r;
        const float upd = mul(lr, gr) / add(sqrtf(r), eps);
        data[i] = fmaxf(sub(data[i], upd), minval);
    } else {
        data[i] = fmaxf(sub(data[i], mul(lr, gr)), minval);
    }
}

}  // namespace
}  // namespace nerf
