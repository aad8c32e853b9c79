// Sparse voxel grid, background layers: the one statement of the march over the spheres, shared by the forward pass
// (grid_background_kernels.hip) and by the taped pass and the backward (grid_background_train_kernels.hip), so that all three
// cross the same spheres with the same fp32 operations - the per-ray set-up, the far hit of a radius, the texel coordinates,
// the cell, the 4 x 2 float4 fetch with its z, y, x interpolation order, the sigma > 0, skip and stop rules.
// Semantics: include/nerf_mi355x.h, "Sparse voxel grid: background layers".
#pragma once
#include "grid_device.h"

namespace nerf {
namespace {

__device__ __forceinline__ float dot3(const float a[3], const float b[3]) {
    return add(add(mul(a[0], b[0]), mul(a[1], b[1])), mul(a[2], b[2]));
}

__device__ __forceinline__ float lerp1(float a, float b, float w) { return add(a, mul(w, sub(b, a))); }

__device__ __forceinline__ float4 lerp4(const float4& a, const float4& b, float w) {
    return make_float4(lerp1(a.x, b.x, w), lerp1(a.y, b.y, w), lerp1(a.z, b.z, w), lerp1(a.w, b.w, w));
}

// row of texel (x, y), or -1
__device__ __forceinline__ int background_link(const GridBg& bg, int x, int y) {
    const int link = bg.links[x * bg.reso + y];
    return (link < 0 || (int64_t)link >= bg.capacity) ? -1 : link;
}

// texel (x, y) between layers lz and lz + 1: zeros without a row
__device__ __forceinline__ float4 background_texel(const GridBg& bg, int x, int y, int lz, float wz) {
    const int link = background_link(bg, x, y);
    if (link < 0) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4* row = reinterpret_cast<const float4*>(bg.data) + ((int64_t)link * bg.nlayers + lz);
    return lerp4(row[0], row[1], wz);
}

// a ray in the normalised box (unit sphere = the first layer) and the constants of its sphere hits
struct BgRay {
    float O[3], D[3];
    float world_step, q2a, qb, two_q2a, f, inner;
};

__device__ __forceinline__ void background_setup(const GridDev& g, const GridRay& rs, BgRay& b) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float s = 2.0f / (float)g.size[i];
        b.O[i] = sub(mul(add(rs.o[i], 0.5f), s), 1.0f);
        b.D[i] = mul(rs.d[i], s);
    }
    const float inorm = 1.0f / sqrtf(dot3(b.D, b.D));
#pragma unroll
    for (int i = 0; i < 3; ++i) b.D[i] = mul(b.D[i], inorm);
    b.world_step = mul(rs.delta_scale, inorm);
    b.q2a = mul(2.0f, dot3(b.D, b.D));
    b.qb = mul(2.0f, dot3(b.O, b.D));
    b.two_q2a = mul(2.0f, b.q2a);
    b.f = sub(mul(b.qb, b.qb), mul(b.two_q2a, dot3(b.O, b.O)));
    const float C[3] = {sub(mul(b.O[1], b.D[2]), mul(b.O[2], b.D[1])), sub(mul(b.O[2], b.D[0]), mul(b.O[0], b.D[2])),
                        sub(mul(b.O[0], b.D[1]), mul(b.O[1], b.D[0]))};
    b.inner = fmaxf(add(sqrtf(dot3(C, C)), 1e-3f), 1.0f);
}

// the sample of one sphere: its cell (with the wrapped neighbours), the weights and 1 / |P|
struct BgSample {
    float invr, wx, wy, wz;
    int lx, ly, lz, nx, ny;
};

// sphere i of n: false where the step is skipped (the radius is inside `inner`, or the ray's line misses the sphere)
__device__ __forceinline__ bool background_sample(const BgRay& b, const GridBg& bg, int n, int i, BgSample& s) {
    constexpr double kInvPi = 0.318309886183790671538;
    const int L = bg.nlayers, R = bg.reso;
    const float rad = (float)((double)n / ((double)(n - i) - 0.5));
    if (rad < b.inner) return false;
    const float det = add(b.f, mul(mul(b.two_q2a, rad), rad));
    if (det < 0.0f) return false;
    const float t = add(-b.qb, sqrtf(det)) / b.q2a;
    const float P[3] = {add(b.O[0], mul(t, b.D[0])), add(b.O[1], mul(t, b.D[1])), add(b.O[2], mul(t, b.D[2]))};
    s.invr = 1.0f / sqrtf(dot3(P, P));
    const float lat = asinf(mul(P[1], s.invr));
    const float lon = atan2f(mul(P[0], s.invr), mul(P[2], s.invr));
    const float x = (float)((double)(2 * R) * (0.5 + ((double)lon * 0.5) * kInvPi));
    const float y = (float)((double)R * (0.5 - (double)lat * kInvPi));
    const float z = fminf(fmaxf(sub(mul(sub(1.0f, s.invr), (float)L), 0.5f), 0.0f), (float)(L - 1));
    // (a NaN coordinate is sent to texel 0 explicitly: nothing may index outside the tables)
    s.lx = x == x ? max(0, min((int)x, 2 * R - 1)) : 0;
    s.ly = y == y ? max(0, min((int)y, R - 1)) : 0;
    s.lz = max(0, min((int)z, L - 2));
    s.wx = sub(x, (float)s.lx);
    s.wy = sub(y, (float)s.ly);
    s.wz = sub(z, (float)s.lz);
    s.nx = s.lx < 2 * R - 1 ? s.lx + 1 : 0;
    s.ny = s.ly < R - 1 ? s.ly + 1 : 0;
    return true;
}

// the 4 x 2 float4 fetch: z first, then y, then x
__device__ __forceinline__ float4 background_fetch(const GridBg& bg, const BgSample& s) {
    const float4 v00 = background_texel(bg, s.lx, s.ly, s.lz, s.wz);
    const float4 v01 = background_texel(bg, s.lx, s.ny, s.lz, s.wz);
    const float4 v10 = background_texel(bg, s.nx, s.ly, s.lz, s.wz);
    const float4 v11 = background_texel(bg, s.nx, s.ny, s.lz, s.wz);
    return lerp4(lerp4(v00, v01, s.wy), lerp4(v10, v11, s.wy), s.wx);
}

// The march of one ray over the n spheres from log_T = log_t: v = fetch(s) at every step that is not skipped, and
// shade(s, v, dstep, weight, log_t after the step) at every shaded step (sigma > 0), in order, with
// dstep = (invr_last - invr) * world_step. Returns the final log_T. n <= 1024 / 1e-3 + 2: the loop ends unconditionally.
template <class Fetch, class Shade>
__device__ __forceinline__ float background_march_fetch(const GridDev& g, const GridBg& bg, const GridRenderOpt& opt, const GridRay& rs,
                                                        float log_t, Fetch&& fetch, Shade&& shade) {
    BgRay b;
    background_setup(g, rs, b);
    float invr_last = 1.0f / b.inner;
    const int n = (int)((float)bg.nlayers / opt.step_size) + 2;
    for (int i = 0; i < n; ++i) {
        BgSample s;
        if (!background_sample(b, bg, n, i, s)) continue;
        const float4 v = fetch(s);
        if (v.w > 0.0f) {
            const float dstep = mul(sub(invr_last, s.invr), b.world_step);
            const float p = mul(dstep, v.w);
            const float weight = mul(expf(log_t), sub(1.0f, expf(-p)));
            log_t = sub(log_t, p);
            shade(s, v, dstep, weight, log_t);
            if (expf(log_t) < opt.stop_thresh) break;
        }
        invr_last = s.invr;
    }
    return log_t;
}

// ... with one lane per ray: the lane fetches all 4 x 2 float4 itself
template <class Shade>
__device__ __forceinline__ float background_march(const GridDev& g, const GridBg& bg, const GridRenderOpt& opt, const GridRay& rs,
                                                  float log_t, Shade&& shade) {
    return background_march_fetch(g, bg, opt, rs, log_t, [&](const BgSample& s) { return background_fetch(bg, s); }, shade);
}

// col_c = v_c * SH_C0 + 0.5: the colour of a channel before its clamp at 0
__device__ __forceinline__ float background_colour(float v) { return add(mul(v, 0.28209479177387814f), 0.5f); }

}  // namespace
}  // namespace nerf
