// Sparse voxel grid: depth maps and ray lengths (svox2's volume_render_depth and return_raylen).
// Semantics: include/nerf_mi355x.h, "Sparse voxel grid: depth and ray lengths". Design and measurements: DESIGN.md section 7g.
//
// Mapping: one lane per ray. A depth march reads densities only - per sample one skip byte, 8 links and at most 8 floats, no
// SH rows - so there is nothing for the render kernel's lanes-per-coefficient to share out: a lane walks its ray alone with
// setup_ray and grid_march of grid_device.h, the functions the render kernel calls (the additions of t and the stall rule,
// march_cell, the skip byte and skip_jump, load_links and sample_sigma are there once, so the sample lattice is the render's,
// bit for bit). No LDS, no scratch, no atomics, no shuffles: every result depends on its own ray only.
// The image form makes its rays in the launch. A wavefront takes an 8 x 8 tile of pixels (lane = 8 * row + column in the
// tile) rather than 64 pixels of a row: the rays of a tile stay within a few cells of one another for the whole march, so the
// wavefront's 64 link and density loads fall on fewer cache lines, and its rays end at more nearly the same sample (less of
// the wavefront idles behind its longest ray). The stores are 8 runs of 32 bytes. (DESIGN.md has the A/B against
// the row mapping.)
#include "grid_device.h"

namespace nerf {
namespace {

constexpr int kTile = 8;      // pixels per side of a wavefront's tile: kTile * kTile = 64 lanes

// the pixel of this thread in row-major order, or -1 outside the image
__device__ __forceinline__ int64_t depth_pixel(const GridCam& cam) {
    const int64_t tid = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    const int64_t tile = tid / (kTile * kTile);
    const int lane = (int)(tid % (kTile * kTile));
    const int tiles_x = (cam.width + kTile - 1) / kTile;
    const int64_t px = (tile % tiles_x) * kTile + lane % kTile;
    const int64_t py = (tile / tiles_x) * kTile + lane / kTile;
    return px < cam.width && py < cam.height ? py * cam.width + px : -1;
}

int64_t depth_image_threads(const GridCam& cam) {
    return (int64_t)((cam.width + kTile - 1) / kTile) * ((cam.height + kTile - 1) / kTile) * (kTile * kTile);
}

template <int MODE, bool IMAGE, bool SKIP>
__global__ __launch_bounds__(kGridThreads) void grid_depth_kernel(GridDev g, GridRenderOpt opt, GridDepth r) {
    int64_t ray;
    GridRay rs;
    if (IMAGE) {
        ray = depth_pixel(r.cam);
        if (ray < 0) return;
        camera_ray(r.cam, ray, rs.o, rs.d);
    } else {
        ray = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
        if (ray >= r.n_rays) return;
        load_ray(r.origins, r.dirs, ray, rs);
    }
    setup_ray<SKIP>(g, opt, rs);
    if (MODE == NERF_GRID_DEPTH_RAYLEN) {
        r.depth[ray] = rs.ok ? sub(rs.tmax, rs.tmin) : __builtin_nanf("");
        return;
    }

    float depth = 0.0f, log_t = 0.0f;
    if (rs.ok && rs.tmin <= rs.tmax) {
        const float world_step = mul(opt.step_size, rs.delta_scale);
        const float neg_step = -opt.step_size;
        grid_march<SKIP>(g, opt, rs, [&](float t, const int*, const float*, const float*, float sigma) {
            if (MODE == NERF_GRID_DEPTH_THRESHOLD) {
                if (!(sigma > r.sigma_thresh)) return false;
                depth = mul(t / opt.step_size, world_step);
                return true;
            }
            if (!(sigma > opt.sigma_thresh)) return false;
            const float a = mul(mul(neg_step, sigma), rs.delta_scale);
            const float weight = mul(expf(log_t), sub(1.0f, expf(a)));
            depth = add(depth, mul(mul(weight, t / opt.step_size), world_step));
            log_t = add(log_t, a);
            if (expf(log_t) < opt.stop_thresh) {
                log_t = -1e3f;
                return true;
            }
            return false;
        });
    }
    r.depth[ray] = depth;
    if (MODE == NERF_GRID_DEPTH_EXPECTED && r.log_transmit) r.log_transmit[ray] = log_t;
}

template <int MODE, bool SKIP>
hipError_t launch_depth_mode(const GridDev& g, const GridRenderOpt& o, const GridDepth& r, hipStream_t s) {
    if (r.origins == nullptr)
        grid_depth_kernel<MODE, true, SKIP><<<blocks_for(depth_image_threads(r.cam)), kGridThreads, 0, s>>>(g, o, r);
    else
        grid_depth_kernel<MODE, false, SKIP><<<blocks_for(r.n_rays), kGridThreads, 0, s>>>(g, o, r);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_grid_depth(const GridDev& g, const GridRenderOpt& o, const GridDepth& r, hipStream_t s) {
    if (r.n_rays <= 0) return hipSuccess;
    const bool skip = g.skip != nullptr;
    switch (r.mode) {
        case NERF_GRID_DEPTH_EXPECTED:
            return skip ? launch_depth_mode<NERF_GRID_DEPTH_EXPECTED, true>(g, o, r, s)
                        : launch_depth_mode<NERF_GRID_DEPTH_EXPECTED, false>(g, o, r, s);
        case NERF_GRID_DEPTH_THRESHOLD:
            return skip ? launch_depth_mode<NERF_GRID_DEPTH_THRESHOLD, true>(g, o, r, s)
                        : launch_depth_mode<NERF_GRID_DEPTH_THRESHOLD, false>(g, o, r, s);
        case NERF_GRID_DEPTH_RAYLEN: return launch_depth_mode<NERF_GRID_DEPTH_RAYLEN, false>(g, o, r, s);      // nothing is marched
    }
    return hipErrorInvalidValue;
}

}  // namespace nerf
