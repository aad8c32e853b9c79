// Sparse voxel grid: the device functions the grid kernels (rendering, training, resampling, components) share, so that all
// walk the same sample lattice with the same fp32 operations: rounded arithmetic, the SH basis, the trilinear set-up, the ray
// set-up and the steps of the march including the skip rule. Semantics: include/nerf_mi355x.h, "Sparse voxel grid".
#pragma once
#include "grid_internal.h"

namespace nerf {
namespace {

constexpr int kGridThreads = 256;

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kGridThreads - 1) / kGridThreads); }      // one thread per item

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

// the 8 links of base cell `base` (corner order 000, 001, 010, ..., 111 = x, y, z bits); anything outside [0, capacity) is -1
__device__ __forceinline__ void load_links(const GridDev& g, int base, int lk[8]) {
    const int sy = g.size[2], sx = g.size[1] * g.size[2];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int v = g.links[base + ((c >> 2) & 1) * sx + ((c >> 1) & 1) * sy + (c & 1)];
        lk[c] = (v >= 0 && (int64_t)v < g.capacity) ? v : -1;
    }
}

// svox2 Camera.gen_rays without NDC: fp64, rounded to fp32 at the end
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
}

// ---- ray set-up (svox2.py:662-693) ----
struct GridRay {
    float o[3], d[3];      // origin and unit direction in grid coordinates
    float v[3];            // unit world direction (the SH argument)
    float delta_scale, tmin, tmax;
    bool ok;               // the set-up is finite: the ray is marched (if tmin <= tmax)
    bool skip_ok;          // skip data may be used (positions exact to 1/16)
};

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

// the sample at t: base cell (returned: its index into links / skip) and trilinear weights
__device__ __forceinline__ int march_cell(const GridDev& g, const GridRay& r, float t, float wa[3], float wb[3]) {
    int l[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        cell_of(add(r.o[i], mul(t, r.d[i])), g.size[i], l[i], wb[i]);
        wa[i] = sub(1.0f, wb[i]);
    }
    return (l[0] * g.size[1] + l[1]) * g.size[2] + l[2];
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

// lane (channel c, coefficient k = col % B): Y_k times the interpolated coefficient, summed over the B lanes of the channel;
// the sum is complete in the lane with k == 0
template <int B>
__device__ __forceinline__ float shade_channel(const GridDev& g, const int lk[8], const float wa[3], const float wb[3], int col,
                                               int k, float yk) {
    float cv[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) cv[c] = lk[c] >= 0 ? g.sh[(int64_t)lk[c] * (3 * B) + col] : 0.0f;
    float part = mul(yk, trilerp(cv, wa, wb));
#pragma unroll
    for (int off = 1; off < B; off <<= 1) {
        const float up = __shfl_down(part, off);
        if (k + off < B) part = add(part, up);
    }
    return part;
}

}  // namespace
}  // namespace nerf
