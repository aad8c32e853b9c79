// C ABI of the sparse voxel grid's depth and ray-length calls (include/nerf_mi355x.h, "Sparse voxel grid: depth and ray
// lengths"): argument checks and the launch. Every check that needs no device comes before the first dereference of the
// handle and before any launch.
#include <cmath>

#include "ctx_internal.h"
#include "grid_internal.h"

using namespace nerf;

namespace {

int depth(const char* fn, nerf_sparse_grid* grid, const nerf_grid_camera* cam, const nerf_grid_render_options* opt,
          const nerf_grid_depth_args* a) {
    int rc = require_grid(fn, grid);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_depth_args);
    GridRenderOpt o{};
    rc = check_grid_options(fn, opt, &o);
    if (rc != NERF_OK) return rc;
    if (a->mode != NERF_GRID_DEPTH_EXPECTED && a->mode != NERF_GRID_DEPTH_THRESHOLD && a->mode != NERF_GRID_DEPTH_RAYLEN) {
        set_error("%s: mode = %d is none of NERF_GRID_DEPTH_EXPECTED, _THRESHOLD, _RAYLEN", fn, a->mode);
        return NERF_E_INVALID;
    }
    if (a->mode == NERF_GRID_DEPTH_THRESHOLD && !(a->sigma_thresh >= 0.0f)) {
        set_error("%s: sigma_thresh = %g must be >= 0 and not NaN (an empty cell must never be a hit)", fn, a->sigma_thresh);
        return NERF_E_INVALID;
    }
    if (a->mode != NERF_GRID_DEPTH_EXPECTED && a->log_transmit) {
        set_error("%s: log_transmit belongs to mode NERF_GRID_DEPTH_EXPECTED, mode = %d", fn, a->mode);
        return NERF_E_INVALID;
    }
    GridDepth r{};
    if (cam) {
        rc = check_grid_camera(fn, cam, &r.cam);
        if (rc != NERF_OK) return rc;
        r.n_rays = (int64_t)cam->width * cam->height;
    } else {
        if (a->n_rays < 0 || a->n_rays > kGridMaxItems || (a->n_rays > 0 && (!a->origins || !a->dirs))) {
            set_error("%s: n_rays = %lld must be in [0, 2^26] and needs origins and dirs", fn, (long long)a->n_rays);
            return NERF_E_INVALID;
        }
        r.origins = a->origins;
        r.dirs = a->dirs;
        r.n_rays = a->n_rays;
    }
    if (r.n_rays > 0 && !a->depth) {
        set_error("%s: depth is NULL", fn);
        return NERF_E_INVALID;
    }
    r.mode = a->mode;
    r.sigma_thresh = a->sigma_thresh;
    r.depth = a->depth;
    r.log_transmit = a->log_transmit;
    GridDev g = grid->g;
    g.skip = a->use_skip ? grid->d_skip : nullptr;
    DeviceGuard dg(grid->ctx->device);
    HIP_TRY(launch_grid_depth(g, o, r, (hipStream_t)a->stream));
    return NERF_OK;
}

}  // namespace

extern "C" {

int nerf_grid_depth_rays(nerf_sparse_grid* grid, const nerf_grid_render_options* opt, const nerf_grid_depth_args* args) {
    return depth("nerf_grid_depth_rays", grid, nullptr, opt, args);
}

int nerf_grid_depth_image(nerf_sparse_grid* grid, const nerf_grid_camera* cam, const nerf_grid_render_options* opt,
                          const nerf_grid_depth_args* args) {
    if (!cam) {
        set_error("nerf_grid_depth_image: nerf_grid_camera is NULL");
        return NERF_E_INVALID;
    }
    return depth("nerf_grid_depth_image", grid, cam, opt, args);
}

}  // extern "C"
