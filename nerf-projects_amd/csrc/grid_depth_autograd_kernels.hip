// Sparse voxel grid, gradients of the expected depth and of log_transmit for autograd: the expected-depth march of
// grid_depth_kernel (grid_depth_kernels.hip) once more with a tape, and its backward with a cotangent for each of the two
// results. Semantics: include/nerf_mi355x.h, "Sparse voxel grid: gradients of depth and log_transmit for autograd". Design,
// generated-code figures and measurements: DESIGN.md section 7i.
//
// All three marches here (taped forward, the backward's look-ahead for the stop, the backward itself) are grid_march of
// grid_device.h, the function grid_depth_kernel calls: setup_ray, the additions of t and the stall rule, march_cell, the skip
// byte and skip_jump, load_links and sample_sigma are there once, so the sample lattice is the forward's by construction.
// Mapping: a ray owns a group of kRayLanes = 32 adjacent lanes in both kernels. Every lane of the group walks the ray - the
// same addresses, so a group's loads are one request, and control flow is uniform inside a group - and in the backward lane c
// of the group's first 8 issues the add of corner c. A batch of a few thousand rays is bound by the latency of its longest
// rays, not by throughput: 5 000 rays at one lane per ray are 79 wavefronts on 256 compute units, each waiting for the
// longest of 64 rays and running the skip and the shade branch one after the other wherever its rays disagree. At 32 lanes
// a wavefront holds 2 rays and the batch 2 500 wavefronts, and a shaded sample costs a wavefront one atomic instruction
// rather than 8. Measured: the backward at 1 / 8 / 16 / 32 lanes per ray takes 1.05 / 0.70 / 0.65 / 0.63 ms
// for 5 000 rays at R = 128, the taped forward 0.52 ms at 1 lane and 0.30 ms at 32.
// Float adds are atomicAdd(float*) = one global_atomic_add_f32 without return (no compare-and-swap loop). No LDS, no
// scratch, no cross-lane operation.
#include "grid_device.h"

namespace nerf {
namespace {

constexpr int kRayLanes = 32;     // adjacent lanes that walk one ray together; the backward's lanes 0..7 add one corner each

template <int GL, bool SKIP>
__global__ __launch_bounds__(kGridThreads) void grid_depth_taped_kernel(GridDev g, GridRenderOpt opt, GridDepthTaped r) {
    const int64_t tid = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    const int64_t ray = tid / GL;
    if (ray >= r.n_rays) return;      // (a whole group leaves together)
    GridRay rs;
    load_ray(r.origins, r.dirs, ray, rs);
    setup_ray<SKIP>(g, opt, rs);

    float depth = 0.0f, log_t = 0.0f;
    double tot = 0.0;      // the depth once more, as the fp64 sum of its fp32 terms: the tape
    if (rs.ok && rs.tmin <= rs.tmax) {
        const float world_step = mul(opt.step_size, rs.delta_scale);
        const float neg_step = -opt.step_size;
        grid_march<SKIP>(g, opt, rs, [&](float t, const int*, const float*, const float*, float sigma) {
            if (!(sigma > opt.sigma_thresh)) return false;
            const float a = mul(mul(neg_step, sigma), rs.delta_scale);
            const float weight = mul(expf(log_t), sub(1.0f, expf(a)));
            const float term = mul(mul(weight, t / opt.step_size), world_step);
            depth = add(depth, term);
            tot += (double)term;
            log_t = add(log_t, a);
            if (expf(log_t) < opt.stop_thresh) {
                log_t = -1e3f;
                return true;
            }
            return false;
        });
    }
    if (tid % GL != 0) return;      // every lane of the group holds the same values: one stores them
    r.depth[ray] = depth;
    r.tape[ray] = tot;
    if (r.log_transmit) r.log_transmit[ray] = log_t;
}

template <int GL, bool SKIP>
__global__ __launch_bounds__(kGridThreads) void grid_depth_bwd_kernel(GridDev g, GridRenderOpt opt, GridDepthBwd r) {
    const int64_t tid = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    const int64_t ray = tid / GL;
    const int lane = (int)(tid % GL);
    if (ray >= r.n_rays) return;      // (a whole group leaves together)
    GridRay rs;
    load_ray(r.origins, r.dirs, ray, rs);
    setup_ray<SKIP>(g, opt, rs);
    if (!(rs.ok && rs.tmin <= rs.tmax)) return;      // a miss or a non-finite set-up: nothing to differentiate

    const float g_d = r.grad_depth ? r.grad_depth[ray] : 0.0f;
    float g_t = r.grad_log_transmit ? r.grad_log_transmit[ray] : 0.0f;
    const float neg_step = -opt.step_size;
    if (g_t != 0.0f && opt.stop_thresh > 0.0f) {
        // a ray that stops returned the constant -1e3: its log_transmit has no gradient. Whether it stops is known only at
        // its end, so such a ray is walked once without adds first.
        float log_t = 0.0f;
        bool stopped = false;
        grid_march<SKIP>(g, opt, rs, [&](float, const int*, const float*, const float*, float sigma) {
            if (!(sigma > opt.sigma_thresh)) return false;
            log_t = add(log_t, mul(mul(neg_step, sigma), rs.delta_scale));
            stopped = expf(log_t) < opt.stop_thresh;
            return stopped;
        });
        if (stopped) g_t = 0.0f;
    }
    if (g_d == 0.0f && g_t == 0.0f) return;      // every term would be zero

    // remaining = what the samples not yet passed still add to the depth: fp64, started from the tape and reduced by the
    // very same fp32 terms that built it, so that it ends at exactly 0 and never carries the cancellation of a fp32 suffix sum
    double remaining = r.tape ? r.tape[ray] : 0.0;
    const float world_step = mul(opt.step_size, rs.delta_scale);
    const float step_ds = world_step;
    float log_t = 0.0f;
    grid_march<SKIP>(g, opt, rs, [&](float t, const int* lk, const float* wa, const float* wb, float sigma) {
        if (!(sigma > opt.sigma_thresh)) return false;
        const float a = mul(mul(neg_step, sigma), rs.delta_scale);
        const float weight = mul(expf(log_t), sub(1.0f, expf(a)));
        const float tau = t / opt.step_size;
        const float term = mul(mul(weight, tau), world_step);
        remaining -= (double)term;
        log_t = add(log_t, a);
        const float lead = mul(mul(expf(log_t), tau), world_step);
        const float d_sigma = sub(mul(step_ds, mul(g_d, sub(lead, (float)remaining))), mul(g_t, step_ds));
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            if (lane != c % GL || lk[c] < 0) continue;
            const float v = mul(corner_weight(c, wa, wb), d_sigma);
            if (v != 0.0f) atomicAdd(&r.grad_density[lk[c]], v);
        }
        return expf(log_t) < opt.stop_thresh;
    });
}

}  // namespace

hipError_t launch_grid_depth_taped(const GridDev& g, const GridRenderOpt& o, const GridDepthTaped& r, hipStream_t s) {
    if (r.n_rays <= 0) return hipSuccess;
    const unsigned blocks = blocks_for(r.n_rays * kRayLanes);
    if (g.skip)
        grid_depth_taped_kernel<kRayLanes, true><<<blocks, kGridThreads, 0, s>>>(g, o, r);
    else
        grid_depth_taped_kernel<kRayLanes, false><<<blocks, kGridThreads, 0, s>>>(g, o, r);
    return hipGetLastError();
}

hipError_t launch_grid_depth_bwd(const GridDev& g, const GridRenderOpt& o, const GridDepthBwd& r, hipStream_t s) {
    if (r.n_rays <= 0) return hipSuccess;
    const unsigned blocks = blocks_for(r.n_rays * kRayLanes);
    if (g.skip)
        grid_depth_bwd_kernel<kRayLanes, true><<<blocks, kGridThreads, 0, s>>>(g, o, r);
    else
        grid_depth_bwd_kernel<kRayLanes, false><<<blocks, kGridThreads, 0, s>>>(g, o, r);
    return hipGetLastError();
}

}  // namespace nerf
