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
// finished or unshaded ray are masked off by EXEC while the other group works. No LDS, no scratch, no atomics (except in the
// instrumented launch that counts samples), 256-thread workgroups and few registers so that every SIMD holds its 8 waves:
// the kernel is bound by the dependent link -> row loads, and waves in flight are what hides them.
#include <algorithm>

#include "grid_internal.h"

namespace nerf {
namespace {

constexpr int kGridThreads = 256;

__device__ __forceinline__ float mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float sub(float a, float b) { return __fsub_rn(a, b); }

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

template <int B, bool IMAGE, bool SKIP, bool COUNT>
__global__ __launch_bounds__(kGridThreads) void grid_render_kernel(GridDev g, GridRenderOpt opt, GridRender r) {
    constexpr int GL = GroupLanes<B>::value;
    const int64_t tid = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    const int64_t ray = tid / GL;
    const int lane = (int)(tid % GL);
    if (ray >= r.n_rays) return;      // (a whole group leaves together)
    const bool busy = lane < 3 * B;
    const int col = busy ? lane : 0;  // idle lanes of a group read column 0 and contribute nothing
    const int k = col % B;

    float o[3], d[3];
    if (IMAGE) {
        camera_ray(r.cam, ray, o, d);
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            o[i] = r.origins[ray * 3 + i];
            d[i] = r.dirs[ray * 3 + i];
        }
    }
    // ---- ray set-up (svox2.py:662-693) ----
    const float dn = sqrtf(add(add(mul(d[0], d[0]), mul(d[1], d[1])), mul(d[2], d[2])));
    float v[3];
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
    const float yk = busy ? sh_basis(k, v[0], v[1], v[2]) : 0.0f;
    // A ray is marched only if its set-up is finite: a zero, NaN or infinite direction or origin is a miss (background,
    // log_transmit 0), whatever fminf / fmaxf made of the NaNs above.
    bool ok = dn > 0.0f && isfinite(dn) && isfinite(delta_scale) && isfinite(tmin) && isfinite(tmax);
    float reach_o = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        ok = ok && isfinite(o[i]) && isfinite(d[i]);
        reach_o = fmaxf(reach_o, fabsf(o[i]));
    }
    // the skip proof (header) needs positions exact to 1/16: |o|, |t| < 2^17 grid units; farther rays march plainly
    const bool skip_ok = SKIP && reach_o < kGridSkipMaxT && fabsf(tmin) < kGridSkipMaxT && fabsf(tmax) < kGridSkipMaxT;

    float outv = 0.0f, log_t = 0.0f;
    unsigned long long visited = 0, shaded = 0;
    if (ok && tmin <= tmax) {
        const float neg_step = -opt.step_size;
        float t = tmin;
        while (t <= tmax) {
            // the march ends unconditionally: every pass through this loop advances t by at least one addition of
            // step_size, and a ray whose t no longer changes under that addition (t so large that step_size is below half
            // an ulp) is left at once
            const float t_next = add(t, opt.step_size);
            if (!(t_next > t)) break;
            int l[3];
            float wa[3], wb[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                cell_of(add(o[i], mul(t, d[i])), g.size[i], l[i], wb[i]);
                wa[i] = sub(1.0f, wb[i]);
            }
            const int base = (l[0] * g.size[1] + l[1]) * g.size[2] + l[2];
            if (SKIP) {
                const int sv = skip_ok ? g.skip[base] : 0;
                if (sv > 0) {
                    // every node within sv - 1 cells of this cell's corners is empty: so are this sample and every later
                    // one whose t (the accumulated value itself, no estimate of it) is within sv - 1 - 1/16 of this one's
                    const float t0 = t, reach = (float)(sv - 1) - 0.0625f;
                    t = t_next;
                    while (sub(t, t0) <= reach) {
                        const float tn = add(t, opt.step_size);
                        if (!(tn > t)) break;
                        t = tn;
                    }
                    continue;
                }
            }
            if (COUNT) ++visited;      // samples whose links are loaded
            int lk[8];
            load_links(g, base, lk);
            float cv[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) cv[c] = lk[c] >= 0 ? g.density[lk[c]] : 0.0f;
            const float sigma = trilerp(cv, wa, wb);
            if (sigma > opt.sigma_thresh) {
                if (COUNT) ++shaded;
#pragma unroll
                for (int c = 0; c < 8; ++c) cv[c] = lk[c] >= 0 ? g.sh[(int64_t)lk[c] * (3 * B) + col] : 0.0f;
                float part = mul(yk, trilerp(cv, wa, wb));
#pragma unroll
                for (int off = 1; off < B; off <<= 1) {
                    const float up = __shfl_down(part, off);
                    if (k + off < B) part = add(part, up);
                }
                const float a = mul(mul(neg_step, sigma), delta_scale);
                const float weight = mul(expf(log_t), sub(1.0f, expf(a)));
                outv = add(outv, mul(weight, fmaxf(add(part, 0.5f), 0.0f)));
                log_t = add(log_t, a);
                if (expf(log_t) < opt.stop_thresh) {
                    log_t = -1e3f;
                    break;
                }
            }
            t = t_next;
        }
    }
    outv = add(outv, mul(expf(log_t), opt.background_brightness));
    if (busy && k == 0) r.rgb[ray * 3 + col / B] = outv;
    if (lane == 0) {
        if (r.log_transmit) r.log_transmit[ray] = log_t;
        if (COUNT) {
            atomicAdd(&r.counters[0], visited);
            atomicAdd(&r.counters[1], shaded);
        }
    }
}

template <int B, bool IMAGE, bool SKIP>
hipError_t launch_render_b(const GridDev& g, const GridRenderOpt& o, const GridRender& r, hipStream_t s) {
    const int64_t threads = r.n_rays * GroupLanes<B>::value;
    const unsigned blocks = (unsigned)((threads + kGridThreads - 1) / kGridThreads);
    if (r.counters)
        grid_render_kernel<B, IMAGE, SKIP, true><<<blocks, kGridThreads, 0, s>>>(g, o, r);
    else
        grid_render_kernel<B, IMAGE, SKIP, false><<<blocks, kGridThreads, 0, s>>>(g, o, r);
    return hipGetLastError();
}

template <int B>
hipError_t launch_render_basis(const GridDev& g, const GridRenderOpt& o, const GridRender& r, hipStream_t s) {
    const bool image = r.origins == nullptr, skip = g.skip != nullptr;
    if (image) return skip ? launch_render_b<B, true, true>(g, o, r, s) : launch_render_b<B, true, false>(g, o, r, s);
    return skip ? launch_render_b<B, false, true>(g, o, r, s) : launch_render_b<B, false, false>(g, o, r, s);
}

// one thread per (point, output column): column 0 = density, 1 + j = SH column j
__global__ __launch_bounds__(kGridThreads) void grid_sample_kernel(GridDev g, const float* __restrict__ points, int64_t n,
                                                                    int grid_coords, int cols, float* __restrict__ density,
                                                                    float* __restrict__ sh) {
    const int64_t tid = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    const int64_t p = tid / cols;
    const int j = (int)(tid % cols);
    if (p >= n) return;
    int l[3];
    float wa[3], wb[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float x = points[p * 3 + i];
        if (!grid_coords) x = add(g.offset[i], mul(x, g.scaling[i]));
        cell_of(x, g.size[i], l[i], wb[i]);
        wa[i] = sub(1.0f, wb[i]);
    }
    int lk[8];
    load_links(g, (l[0] * g.size[1] + l[1]) * g.size[2] + l[2], lk);
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
    const int kz = (int)(idx % g.size[2]), jy = (int)((idx / g.size[2]) % g.size[1]), ix = (int)(idx / ((int64_t)g.size[2] * g.size[1]));
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

unsigned blocks_for(int64_t n) { return (unsigned)((n + kGridThreads - 1) / kGridThreads); }

}  // namespace

hipError_t launch_grid_render(const GridDev& g, const GridRenderOpt& o, const GridRender& r, hipStream_t s) {
    if (r.n_rays <= 0) return hipSuccess;
    switch (g.basis_dim) {
        case 9: return launch_render_basis<9>(g, o, r, s);
        case 4: return launch_render_basis<4>(g, o, r, s);
        case 1: return launch_render_basis<1>(g, o, r, s);
    }
    return hipErrorInvalidValue;
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
