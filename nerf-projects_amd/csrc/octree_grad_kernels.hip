// PlenOctree: the gradient of a march with respect to the rows of `data`, and the fused clamped-MSE form.
// Semantics: include/nerf_mi355x.h, "PlenOctree: backward". Design and measurements: DESIGN.md section 7t,
// profiles/octree_train.md.
//
// One lane per ray, as in the renderer, and no tape: the geometry of a march (leaves, delta) depends on `child` and the ray
// alone, so the kernel marches twice. Pass 1 is the renderer's loop, operation for operation (octree_device.h holds what
// both share): it gives the renderer's rgb bits, the unscaled sums A_c, the final transmittance T_e, whether the ray stopped
// at stop_thresh and the pass of the last shaded leaf. Pass 2 marches again from the front up to that leaf with the running
// prefix pre_c and emits, per shaded leaf, the D = 3 B + 1 entries of its row's gradient.
// The scatter: lanes of a wavefront sit in 64 different rows, the slow shape for float atomics. Per march pass the lanes with
// a shaded leaf stage their D values in a lane-private LDS row; the wavefront then walks the ballot of those lanes and adds
// each staged row to grad_data as one contiguous segment of D floats (two rows per instruction where D <= 32: lanes 0-31
// one row, lanes 32-63 the next). A block is one wavefront, so the staging needs no barrier between waves. Every lane adding
// its own entries instead measured 8 times this kernel's frame (profiles/octree_train.md; that form is kept as
// profiles/microbench/octree_lane_scatter.patch).
#include "grid_device.h"
#include "octree_device.h"
#include "octree_internal.h"

namespace nerf {
namespace {

constexpr int kWave = 64;

template <int B, bool IMAGE, bool ACCEL, bool FUSED>
__global__ __launch_bounds__(kWave) void octree_backward_kernel(OctreeDev t, OctreeRenderOpt opt, OctreeBackward r) {
    constexpr int D = 3 * B + 1;
    constexpr int kStride = D | 1;      // odd: 64 lanes writing entry j of their rows hit 64 banks
    __shared__ float stage[kWave * kStride];
    const int lane = (int)threadIdx.x;
    const int64_t tid = (int64_t)blockIdx.x * kWave + threadIdx.x;
    // no lane leaves early: the loss sum and the flush are wavefront-wide
    int64_t ray;
    float ow[3] = {0.0f, 0.0f, 0.0f}, dw[3] = {0.0f, 0.0f, 0.0f};
    bool valid;
    if (IMAGE) {
        ray = tile_pixel(r.cam, tid);
        valid = ray >= 0;
        if (valid) camera_ray(r.cam, ray, ow, dw);
    } else {
        ray = tid;
        valid = ray < r.n_rays;
        if (valid) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                ow[i] = r.origins[ray * 3 + i];
                dw[i] = r.dirs[ray * 3 + i];
            }
        }
    }
    OctreeRay rs;
    octree_setup(t, ow, dw, rs);
    float basis[B];
    octree_sh_basis<B>(dw[0], dw[1], dw[2], basis);
    const float hi = sub(1.0f, 1e-6f);
    const bool enters = valid && rs.ok && !(rs.tmax < 0.0f) && !(rs.tmin > rs.tmax);

    // ---- pass 1: the renderer's march ----
    float A[3] = {0.0f, 0.0f, 0.0f};
    float T = 1.0f;
    int steps = 0, last = 0;      // last: the pass of the last shaded leaf
    bool stopped = false;
    if (enters) {
        float tt = rs.tmin;
        while (tt < rs.tmax) {
            if (steps >= kOctreeMaxIters) {
                if (r.capped) atomicAdd(r.capped, 1ull);
                break;
            }
            ++steps;
            float p[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) p[i] = fminf(fmaxf(add(rs.o[i], mul(tt, rs.d[i])), 0.0f), hi);
            float inv_cube;
            const int64_t cell = octree_descend<ACCEL>(t, p, inv_cube);
            float a, b;
            unit_cube(p, rs.inv, a, b);
            const float delta = add(mul(sub(b, a), inv_cube), opt.step_size);
            const float* row = t.data + cell * t.data_dim;
            const float sigma = row[3 * B];
            if (sigma > opt.sigma_thresh) {
                const float att = expf(mul(mul(-delta, rs.delta_scale), sigma));
                const float weight = mul(T, sub(1.0f, att));
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float s = mul(basis[0], row[c * B]);
#pragma unroll
                    for (int i = 1; i < B; ++i) s = add(s, mul(basis[i], row[c * B + i]));
                    A[c] = add(A[c], mul(weight, octree_act(t.act, s)));
                }
                T = mul(T, att);
                last = steps;
                if (T <= opt.stop_thresh) {
                    stopped = true;
                    break;
                }
            }
            const float tn = add(tt, delta);
            if (!(tn > tt)) break;
            tt = tn;
        }
    }
    const float scale = stopped ? __fdiv_rn(1.0f, sub(1.0f, T)) : 1.0f;
    float rgb[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        rgb[c] = stopped ? mul(A[c], scale) : add(A[c], mul(T, opt.background_brightness));
        if (!rs.ok) rgb[c] = __builtin_nanf("");
    }
    if (valid && r.rgb) {
#pragma unroll
        for (int c = 0; c < 3; ++c) r.rgb[ray * 3 + c] = rgb[c];
    }

    // ---- the incoming gradient; the loss, summed over the wavefront before its one atomic ----
    float g[3] = {0.0f, 0.0f, 0.0f};
    float lsum = 0.0f;
    if (valid && rs.ok) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (FUSED) {
                const float diff = fminf(fmaxf(rgb[c], 0.0f), 1.0f) - r.rgb_gt[ray * 3 + c];
                lsum += diff * diff;
                g[c] = rgb[c] >= 0.0f && rgb[c] <= 1.0f ? r.loss_scale * diff : 0.0f;      // torch.clamp's closed interval
            } else {
                g[c] = r.grad_rgb[ray * 3 + c];
            }
        }
    }
    if (FUSED && r.loss) {
#pragma unroll
        for (int m = kWave / 2; m >= 1; m >>= 1) lsum += __shfl_xor(lsum, m);
        if (lane == 0 && lsum != 0.0f) atomicAdd(r.loss, lsum);
    }

    // ---- pass 2: front to back again, up to the last shaded leaf ----
    // U_c: the unscaled colour, background included; what lies behind leaf k is U_c - pre_c - w_k col_kc
    float U[3], gs[3], pre[3] = {0.0f, 0.0f, 0.0f};
    float gA = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        U[c] = stopped ? A[c] : rgb[c];
        gs[c] = g[c] * scale;
        gA += g[c] * A[c];
    }
    const float stop_term = stopped ? -gA * scale * scale * T : 0.0f;
    bool live = enters && last > 0 && (g[0] != 0.0f || g[1] != 0.0f || g[2] != 0.0f);
    float tt = rs.tmin, Tk = 1.0f;
    int step = 0;
    while (__any(live)) {      // one march pass of every live lane, then the wavefront's flush
        bool shaded = false;
        int cell32 = 0;      // (cell indices stay below 2^30)
        if (live) {
            ++step;
            float p[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) p[i] = fminf(fmaxf(add(rs.o[i], mul(tt, rs.d[i])), 0.0f), hi);
            float inv_cube;
            const int64_t cell = octree_descend<ACCEL>(t, p, inv_cube);
            float a, b;
            unit_cube(p, rs.inv, a, b);
            const float delta = add(mul(sub(b, a), inv_cube), opt.step_size);
            const float* row = t.data + cell * t.data_dim;
            const float sigma = row[3 * B];
            if (sigma > opt.sigma_thresh) {
                shaded = true;
                cell32 = (int)cell;
                const float len = mul(delta, rs.delta_scale);
                const float att = expf(mul(mul(-delta, rs.delta_scale), sigma));
                const float w = mul(Tk, sub(1.0f, att));
                const float Ta = Tk * att;
                float* out = stage + lane * kStride;
                float acc = stop_term;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float s = mul(basis[0], row[c * B]);
#pragma unroll
                    for (int i = 1; i < B; ++i) s = add(s, mul(basis[i], row[c * B + i]));
                    const float col = octree_act(t.act, s);
                    const float dact = t.act == NERF_OCTREE_RGB_RELU_HALF ? (add(s, 0.5f) > 0.0f ? 1.0f : 0.0f) : col * (1.0f - col);
                    const float wc = mul(w, col);
                    acc += gs[c] * (Ta * col - ((U[c] - pre[c]) - wc));
                    const float k = gs[c] * w * dact;
#pragma unroll
                    for (int i = 0; i < B; ++i) out[c * B + i] = k * basis[i];
                    pre[c] = add(pre[c], wc);
                }
                out[3 * B] = len * acc;
                Tk = mul(Tk, att);
            }
            if (step >= last) live = false;
            else tt = add(tt, delta);      // (pass 1 went on from here, so the step is not lost below an ulp of tt)
        }
        unsigned long long mask = __ballot(shaded);
        if (mask) {      // (the same in every lane)
            __syncthreads();
            while (mask) {
                const int s0 = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                int src = s0, j = lane;
                if (D <= kWave / 2) {      // two rows per instruction
                    int s1 = -1;
                    if (mask) {
                        s1 = __ffsll((long long)mask) - 1;
                        mask &= mask - 1;
                    }
                    src = lane < kWave / 2 ? s0 : s1;
                    j = lane % (kWave / 2);
                }
                const int dst = __shfl(cell32, src < 0 ? 0 : src);
#pragma unroll
                for (int j0 = 0; j0 < D; j0 += kWave) {
                    if (src >= 0 && j0 + j < D) {
                        const float v = stage[src * kStride + j0 + j];
                        if (v != 0.0f) atomicAdd(r.grad_data + (int64_t)dst * D + j0 + j, v);      // adds of exact zeros are skipped
                    }
                }
            }
            __syncthreads();
        }
    }
}

template <class F>
hipError_t with_flag(bool v, F&& f) {
    return v ? f(std::true_type()) : f(std::false_type());
}

}  // namespace

hipError_t launch_octree_backward(const OctreeDev& t, const OctreeRenderOpt& o, const OctreeBackward& b, hipStream_t s) {
    if (b.n_rays <= 0) return hipSuccess;
    return dispatch_octree_basis(t.basis_dim, [&](auto bd) {
        constexpr int B = decltype(bd)::value;
        const bool image = b.origins == nullptr;
        const int64_t threads = image ? image_threads(b.cam) : b.n_rays;
        const unsigned blocks = (unsigned)((threads + kWave - 1) / kWave);      // one wavefront a block
        return with_flag(image, [&](auto im) {
            return with_flag(t.table != nullptr, [&](auto ac) {
                return with_flag(b.rgb_gt != nullptr, [&](auto fu) {
                    octree_backward_kernel<B, decltype(im)::value, decltype(ac)::value, decltype(fu)::value>
                        <<<blocks, kWave, 0, s>>>(t, o, b);
                    return hipGetLastError();
                });
            });
        });
    });
}

}  // namespace nerf
