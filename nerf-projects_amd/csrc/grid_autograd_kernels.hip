// Sparse voxel grid, gradients for autograd: the two marches of grid_fused_kernel (grid_train_kernels.hip) as kernels of their
// own, with the cotangent d loss / d rgb read from memory between them, and the transpose of grid_sample_kernel. Semantics:
// include/nerf_mi355x.h, "Sparse voxel grid: gradients for autograd". Design, generated-code figures and measurements:
// DESIGN.md section 7h.
//
// Both render kernels keep the lane layout of grid_render_kernel (grid_device.h): one SH coefficient per lane, a ray owns a
// group of 32 / 16 / 4 lanes at basis_dim 9 / 4 / 1, control flow uniform inside a group. grid_taped_kernel is the first
// march of grid_fused_kernel operation for operation and leaves, besides the colour, the tape: per ray and channel the
// colour as the fp64 sum of its exact weight * colour products plus the background term (24 B per ray). grid_render_bwd_kernel
// is the second march: `remaining` starts from the tape, g_c comes from grad_rgb, and at every shaded sample lane (c, k) adds
// w8 * (weight * Y_k * g_c) to grad_sh[row, c * B + k] while lanes 0..7 of the group (0..3 twice at basis_dim 1) each take
// one corner's density add and mask byte. A table whose pointer is NULL gets nothing: the test is uniform over the launch.
// Float adds are atomicAdd(float*) = one global_atomic_add_f32 without return (no compare-and-swap loop); the mask is
// written with plain byte stores (every writer stores 1). No LDS, no scratch.
#include "grid_device.h"

namespace nerf {
namespace {

// weight of corner c (x, y, z bits) = wx * wy * wz, in that order
__device__ __forceinline__ float corner_weight(int c, const float wa[3], const float wb[3]) {
    return mul(mul((c & 4) ? wb[0] : wa[0], (c & 2) ? wb[1] : wa[1]), (c & 1) ? wb[2] : wa[2]);
}

template <int B, bool SKIP>
__global__ __launch_bounds__(kGridThreads) void grid_taped_kernel(GridDev g, GridRenderOpt opt, GridTaped r) {
    constexpr int GL = GroupLanes<B>::value;
    const int64_t tid = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    const int64_t ray = tid / GL;
    const int lane = (int)(tid % GL);
    if (ray >= r.n_rays) return;      // (a whole group leaves together)
    const bool busy = lane < 3 * B;
    const int col = busy ? lane : 0;  // idle lanes of a group read column 0 and contribute nothing
    const int k = col % B;

    GridRay rs;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        rs.o[i] = r.origins[ray * 3 + i];
        rs.d[i] = r.dirs[ray * 3 + i];
    }
    setup_ray<SKIP>(g, opt, rs);
    const float yk = busy ? sh_basis(k, rs.v[0], rs.v[1], rs.v[2]) : 0.0f;
    const bool marched = rs.ok && rs.tmin <= rs.tmax;
    const float neg_step = -opt.step_size;

    float outv = 0.0f, log_t = 0.0f;
    double tot = 0.0;      // the channel's colour once more, as the exact sum of its terms: the tape
    if (marched) {
        float t = rs.tmin;
        while (t <= rs.tmax) {
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
            const float sigma = sample_sigma(g, lk, wa, wb);
            if (sigma > opt.sigma_thresh) {
                const float part = shade_channel<B>(g, lk, wa, wb, col, k, yk);
                const float a = mul(mul(neg_step, sigma), rs.delta_scale);
                const float weight = mul(expf(log_t), sub(1.0f, expf(a)));
                const float colour = fmaxf(add(part, 0.5f), 0.0f);
                outv = add(outv, mul(weight, colour));
                tot += (double)weight * (double)colour;      // (a product of two floats is exact in a double)
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
    tot += (double)expf(log_t) * (double)opt.background_brightness;
    if (busy && k == 0) {      // the lanes in which the channel's sum is complete
        r.rgb[ray * 3 + col / B] = outv;
        r.tape[ray * 3 + col / B] = tot;
    }
    if (lane == 0 && r.log_transmit) r.log_transmit[ray] = log_t;
}

template <int B, bool SKIP>
__global__ __launch_bounds__(kGridThreads) void grid_render_bwd_kernel(GridDev g, GridRenderOpt opt, GridRenderBwd r) {
    constexpr int GL = GroupLanes<B>::value;
    constexpr int DL = GL < 8 ? GL : 8;      // lanes of a group that share the 8 density adds
    const int64_t tid = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    const int64_t ray = tid / GL;
    const int lane = (int)(tid % GL);
    if (ray >= r.n_rays) return;
    const bool busy = lane < 3 * B;
    const int col = busy ? lane : 0;
    const int k = col % B;

    GridRay rs;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        rs.o[i] = r.origins[ray * 3 + i];
        rs.d[i] = r.dirs[ray * 3 + i];
    }
    setup_ray<SKIP>(g, opt, rs);
    if (!(rs.ok && rs.tmin <= rs.tmax)) return;      // a miss or a non-finite set-up: nothing to differentiate
    const float yk = busy ? sh_basis(k, rs.v[0], rs.v[1], rs.v[2]) : 0.0f;
    const float neg_step = -opt.step_size;

    // remaining[c] = what the samples not yet passed, and the background, still add to channel c: fp64, started from the
    // tape and reduced by the very same exact products that built it (grid_train_kernels.hip says why)
    float gc[3];
    double remaining[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        gc[c] = r.grad_rgb[ray * 3 + c];
        remaining[c] = r.tape[ray * 3 + c];
    }
    const float g_own = col / B == 0 ? gc[0] : (col / B == 1 ? gc[1] : gc[2]);
    const float step_ds = mul(opt.step_size, rs.delta_scale);
    const bool want_sh = busy && r.grad_sh != nullptr;
    const bool want_density = r.grad_density != nullptr, want_mask = r.mask != nullptr;

    float log_t = 0.0f;
    float t = rs.tmin;
    while (t <= rs.tmax) {
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
        const float sigma = sample_sigma(g, lk, wa, wb);
        if (sigma > opt.sigma_thresh) {
            const float part = shade_channel<B>(g, lk, wa, wb, col, k, yk);
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
                if (col / B == c) raw_own = rc;
            }
            const float accum = (float)accum64;
            const float d_sigma = mul(step_ds, sub(mul(expf(log_t), dot), accum));
            // max(0, .) passes the gradient where its argument is >= 0 (torch.clamp_min)
            const float d_coef = raw_own >= 0.0f ? mul(mul(weight, yk), g_own) : 0.0f;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                if (lk[c] < 0) continue;
                const float w8 = corner_weight(c, wa, wb);
                if (want_sh) {
                    const float v = mul(w8, d_coef);
                    if (v != 0.0f) atomicAdd(&r.grad_sh[(int64_t)lk[c] * (3 * B) + col], v);
                }
                if (lane == c % DL) {
                    if (want_density) atomicAdd(&r.grad_density[lk[c]], mul(w8, d_sigma));
                    if (want_mask) r.mask[lk[c]] = 1;
                }
            }
            if (expf(log_t) < opt.stop_thresh) break;
        }
        t = t_next;
    }
}

// The transpose of grid_sample_kernel: one thread per (point, column), column 0 = density. The cell, the weights and the
// world -> grid transform are that kernel's; corner (x, y, z bits) of a kept link receives ((w_x * go) * w_y) * w_z.
__global__ __launch_bounds__(kGridThreads) void grid_sample_bwd_kernel(GridDev g, GridSampleBwd a, int cols) {
    const int64_t tid = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    const int64_t p = tid / cols;
    const int j = (int)(tid % cols);
    if (p >= a.n) return;
    const int row = 3 * g.basis_dim;
    float* table = j == 0 ? a.grad_density : a.grad_sh;
    if (!table) return;
    const float go = j == 0 ? a.grad_out_density[p] : a.grad_out_sh[p * row + (j - 1)];
    int l[3];
    float wa[3], wb[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float x = a.points[p * 3 + i];
        if (!a.grid_coords) x = add(g.offset[i], mul(x, g.scaling[i]));
        cell_of(x, g.size[i], l[i], wb[i]);
        wa[i] = sub(1.0f, wb[i]);
    }
    int lk[8];
    load_links(g, (l[0] * g.size[1] + l[1]) * g.size[2] + l[2], lk);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        if (lk[c] < 0) continue;
        const float v = mul(mul(mul((c & 4) ? wb[0] : wa[0], go), (c & 2) ? wb[1] : wa[1]), (c & 1) ? wb[2] : wa[2]);
        if (v != 0.0f) atomicAdd(j == 0 ? &table[lk[c]] : &table[(int64_t)lk[c] * row + (j - 1)], v);
    }
}

template <int B>
hipError_t launch_taped_b(const GridDev& g, const GridRenderOpt& o, const GridTaped& r, hipStream_t s) {
    const unsigned blocks = blocks_for(r.n_rays * GroupLanes<B>::value);
    if (g.skip)
        grid_taped_kernel<B, true><<<blocks, kGridThreads, 0, s>>>(g, o, r);
    else
        grid_taped_kernel<B, false><<<blocks, kGridThreads, 0, s>>>(g, o, r);
    return hipGetLastError();
}

template <int B>
hipError_t launch_bwd_b(const GridDev& g, const GridRenderOpt& o, const GridRenderBwd& r, hipStream_t s) {
    const unsigned blocks = blocks_for(r.n_rays * GroupLanes<B>::value);
    if (g.skip)
        grid_render_bwd_kernel<B, true><<<blocks, kGridThreads, 0, s>>>(g, o, r);
    else
        grid_render_bwd_kernel<B, false><<<blocks, kGridThreads, 0, s>>>(g, o, r);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_grid_render_taped(const GridDev& g, const GridRenderOpt& o, const GridTaped& r, hipStream_t s) {
    if (r.n_rays <= 0) return hipSuccess;
    switch (g.basis_dim) {
        case 9: return launch_taped_b<9>(g, o, r, s);
        case 4: return launch_taped_b<4>(g, o, r, s);
        case 1: return launch_taped_b<1>(g, o, r, s);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_grid_render_bwd(const GridDev& g, const GridRenderOpt& o, const GridRenderBwd& r, hipStream_t s) {
    if (r.n_rays <= 0) return hipSuccess;
    switch (g.basis_dim) {
        case 9: return launch_bwd_b<9>(g, o, r, s);
        case 4: return launch_bwd_b<4>(g, o, r, s);
        case 1: return launch_bwd_b<1>(g, o, r, s);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_grid_sample_bwd(const GridDev& g, const GridSampleBwd& a, hipStream_t s) {
    const int cols = a.want_colors ? 1 + 3 * g.basis_dim : 1;
    if (a.n <= 0) return hipSuccess;
    grid_sample_bwd_kernel<<<blocks_for(a.n * cols), kGridThreads, 0, s>>>(g, a, cols);
    return hipGetLastError();
}

}  // namespace nerf
