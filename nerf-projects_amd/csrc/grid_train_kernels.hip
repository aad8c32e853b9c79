// Sparse voxel grid (Plenoxels) training kernels: the fused render + MSE backward, the total-variation gradient over a range
// of cells, and the masked RMSProp / SGD step. Semantics: include/nerf_mi355x.h, "Sparse voxel grid: training". Design,
// generated-code figures and measurements: DESIGN.md section 7d.
//
// grid_fused_kernel keeps the lane layout of grid_render_kernel (grid_device.h): one SH coefficient per lane, a ray owns a
// group of 32 / 16 / 4 lanes at basis_dim 9 / 4 / 1. A ray is marched twice by its group. The first march is the render
// itself, operation for operation, and leaves the colour in registers (channel c in the group's lane c * B); nothing goes
// through memory between the two. The second march walks the same lattice - the same fp32 additions of t, the same skip
// data, the same sigma_thresh and stop rules - and at every shaded sample scatters the gradients into the 8 corner rows:
// lane (c, k) adds w8 * (weight * Y_k * g_c) to grad_sh[row, c * B + k], so a corner's 12 B * B gradient row is one
// contiguous run of float atomics issued by the group in one instruction, and lanes 0..7 of the group (0..3 twice at
// basis_dim 1) each take one corner's density add and mask byte. The per-sample colour of all three channels, which every
// lane needs for d sigma, is spread with three group-wide shuffles. Control flow is uniform inside a group; groups of a
// wavefront diverge exactly as they do in the renderer.
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
__global__ __launch_bounds__(kGridThreads) void grid_fused_kernel(GridDev g, GridRenderOpt opt, GridFused r) {
    constexpr int GL = GroupLanes<B>::value;
    constexpr int DL = GL < 8 ? GL : 8;      // lanes of a group that share the 8 density adds
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

    // ---- first march: grid_render_kernel's loop ----
    float outv = 0.0f, log_t = 0.0f;
    double tot = 0.0;      // the channel's colour once more, as the exact sum of its terms (for `remaining` below)
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
    if (busy && k == 0) r.rgb[ray * 3 + col / B] = outv;
    if (lane == 0 && r.log_transmit) r.log_transmit[ray] = log_t;
    if (!marched) return;      // a miss or a non-finite set-up: nothing to differentiate

    // ---- d loss / d rgb: every lane holds all three channels ----
    // remaining[c] = what the samples not yet passed, and the background, still add to channel c. It is the one quantity of
    // the backward that is a difference of large, nearly equal sums (the colour minus what the passed samples gave); in fp32
    // its rounding, 6e-8 of the whole colour, is a relative 1e-3 of the small density gradients behind a bright sample, which
    // RMSProp's g / (sqrt(rms) + eps) turns into density errors of 1e-3. Kept in fp64, built from and reduced by the very
    // same exact products, it is exact to 1e-16 of the colour; everything else is fp32.
    float gc[3];
    double remaining[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float rgb = __shfl(outv, c * B, GL);
        gc[c] = mul(sub(rgb, r.rgb_gt[ray * 3 + c]), r.grad_scale);
        remaining[c] = __shfl(tot, c * B, GL);      // (the background term is part of it)
    }
    const float g_own = col / B == 0 ? gc[0] : (col / B == 1 ? gc[1] : gc[2]);
    const float step_ds = mul(opt.step_size, rs.delta_scale);

    // ---- second march: the same lattice, gradients scattered ----
    log_t = 0.0f;
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
                if (busy) {
                    const float v = mul(w8, d_coef);
                    if (v != 0.0f) atomicAdd(&r.grad_sh[(int64_t)lk[c] * (3 * B) + col], v);
                }
                if (lane == c % DL) {
                    atomicAdd(&r.grad_density[lk[c]], mul(w8, d_sigma));
                    r.mask[lk[c]] = 1;
                }
            }
            if (expf(log_t) < opt.stop_thresh) break;
        }
        t = t_next;
    }
}

template <int B>
hipError_t launch_fused_b(const GridDev& g, const GridRenderOpt& o, const GridFused& r, hipStream_t s) {
    const int64_t threads = r.n_rays * GroupLanes<B>::value;
    const unsigned blocks = (unsigned)((threads + kGridThreads - 1) / kGridThreads);
    if (g.skip)
        grid_fused_kernel<B, true><<<blocks, kGridThreads, 0, s>>>(g, o, r);
    else
        grid_fused_kernel<B, false><<<blocks, kGridThreads, 0, s>>>(g, o, r);
    return hipGetLastError();
}

// One thread per (cell of the range, column): svox2's tv_grad_sparse_kernel with ignore_edge = 0, ignore_last_z = 0, no NDC.
// Cell i of the range is node (start + i) mod X Y Z; forward differences to its +x, +y, +z neighbours, an empty or
// out-of-range node counts as 0 and receives nothing.
__global__ __launch_bounds__(kGridThreads) void grid_tv_grad_kernel(GridDev g, GridTv a) {
    const int ncol = a.end_dim - a.start_dim;
    const int64_t tid = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    const int64_t i = tid / ncol;
    if (i >= a.count) return;
    const int col = (int)(tid % ncol) + a.start_dim;
    const int64_t n = (int64_t)g.size[0] * g.size[1] * g.size[2];
    const int64_t cell = (a.start + i) % n;
    int x, y, z;
    node_to_xyz(cell, g.size, x, y, z);
    const int sy = g.size[2], sx = g.size[1] * g.size[2];
    int lk[4];      // 000, +x, +y, +z
    lk[0] = g.links[cell];
    lk[1] = x + 1 < g.size[0] ? g.links[cell + sx] : -1;
    lk[2] = y + 1 < g.size[1] ? g.links[cell + sy] : -1;
    lk[3] = z + 1 < g.size[2] ? g.links[cell + 1] : -1;
    float v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (!(lk[c] >= 0 && (int64_t)lk[c] < g.capacity)) lk[c] = -1;
        v[c] = lk[c] >= 0 ? a.data[(int64_t)lk[c] * a.cols + col] : 0.0f;
    }
    float dx = sub(v[1], v[0]), dy = sub(v[2], v[0]), dz = sub(v[3], v[0]);
    const float ss = add(add(add(1e-9f, mul(dx, dx)), mul(dy, dy)), mul(dz, dz));
    const float idelta = a.scale / sqrtf(ss);
    dx = mul(dx, a.axis_scale[0]);
    dy = mul(dy, a.axis_scale[1]);
    dz = mul(dz, a.axis_scale[2]);
    const float val[4] = {-add(add(dx, dy), dz), dx, dy, dz};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (lk[c] >= 0 && val[c] != 0.0f) {
            atomicAdd(&a.grad[(int64_t)lk[c] * a.cols + col], mul(val[c], idelta));
            a.mask[lk[c]] = 1;
        }
    }
}

// svox2's rmsprop_mask_step_kernel / sgd_mask_step_kernel, one thread per element of the rows whose mask byte is set. Every
// operation is one rounded fp32 operation, in the order written (include/nerf_mi355x.h states it).
template <bool RMSPROP>
__global__ __launch_bounds__(kGridThreads) void grid_optim_step_kernel(GridOptim a) {
    const int64_t tid = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (tid >= a.rows * a.cols) return;
    if (!a.mask[tid / a.cols]) return;
    const float gr = a.grad[tid];
    if (RMSPROP) {
        const float g2 = mul(gr, gr);
        float rms = a.rms[tid];
        rms = rms == 0.0f ? g2 : add(g2, mul(a.beta, sub(rms, g2)));
        a.rms[tid] = rms;
        const float upd = mul(a.lr, gr) / add(sqrtf(rms), a.eps);
        a.data[tid] = fmaxf(sub(a.data[tid], upd), a.minval);
    } else {
        a.data[tid] = fmaxf(sub(a.data[tid], mul(a.lr, gr)), a.minval);
    }
}

}  // namespace

hipError_t launch_grid_fused(const GridDev& g, const GridRenderOpt& o, const GridFused& r, hipStream_t s) {
    if (r.n_rays <= 0) return hipSuccess;
    switch (g.basis_dim) {
        case 9: return launch_fused_b<9>(g, o, r, s);
        case 4: return launch_fused_b<4>(g, o, r, s);
        case 1: return launch_fused_b<1>(g, o, r, s);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_grid_tv_grad(const GridDev& g, const GridTv& a, hipStream_t s) {
    const int64_t n = a.count * (a.end_dim - a.start_dim);
    if (n <= 0) return hipSuccess;
    grid_tv_grad_kernel<<<blocks_for(n), kGridThreads, 0, s>>>(g, a);
    return hipGetLastError();
}

hipError_t launch_grid_optim_step(const GridOptim& a, int rmsprop, hipStream_t s) {
    const int64_t n = a.rows * a.cols;
    if (n <= 0) return hipSuccess;
    if (rmsprop)
        grid_optim_step_kernel<true><<<blocks_for(n), kGridThreads, 0, s>>>(a);
    else
        grid_optim_step_kernel<false><<<blocks_for(n), kGridThreads, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace nerf
