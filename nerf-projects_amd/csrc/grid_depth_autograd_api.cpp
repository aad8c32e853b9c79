// C ABI of the gradients of the sparse voxel grid's depth and log_transmit (include/nerf_mi355x.h, "Sparse voxel grid:
// gradients of depth and log_transmit for autograd"): argument checks and the launches. Every check that needs no device
// comes before the first dereference of the handle and before any launch.
#include "ctx_internal.h"
#include "grid_internal.h"

using namespace nerf;

namespace {

int check_rays(const char* fn, int64_t n_rays, const float* origins, const float* dirs) {
    if (n_rays < 0 || n_rays > kGridMaxItems || (n_rays > 0 && (!origins || !dirs))) {
        set_error("%s: n_rays = %lld must be in [0, 2^26] and needs origins and dirs", fn, (long long)n_rays);
        return NERF_E_INVALID;
    }
    return NERF_OK;
}

}  // namespace

extern "C" {

int nerf_grid_depth_rays_taped(nerf_sparse_grid* grid, const nerf_grid_render_options* opt, const nerf_grid_depth_taped_args* a) {
    const char* fn = "nerf_grid_depth_rays_taped";
    int rc = require_grid(fn, grid);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_depth_taped_args);
    GridRenderOpt o{};
    rc = check_grid_options(fn, opt, &o);
    if (rc != NERF_OK) return rc;
    rc = check_rays(fn, a->n_rays, a->origins, a->dirs);
    if (rc != NERF_OK) return rc;
    if (a->n_rays > 0 && !a->depth) {
        set_error("%s: depth is NULL", fn);
        return NERF_E_INVALID;
    }
    if (a->n_rays > 0 && !a->tape) {
        set_error("%s: tape is NULL", fn);
        return NERF_E_INVALID;
    }
    if (a->n_rays == 0) return NERF_OK;
    rc = refuse_palette_grid(fn, grid);      // (the first read of the handle)
    if (rc != NERF_OK) return rc;
    GridDepthTaped r{a->origins, a->dirs, a->n_rays, a->depth, a->log_transmit, a->tape};
    GridDev g = grid->g;
    g.skip = a->use_skip ? grid->d_skip : nullptr;
    DeviceGuard dg(grid->ctx->device);
    HIP_TRY(launch_grid_depth_taped(g, o, r, (hipStream_t)a->stream));
    return NERF_OK;
}

int nerf_grid_depth_backward(nerf_sparse_grid* grid, const nerf_grid_render_options* opt, const nerf_grid_depth_backward_args* a) {
    const char* fn = "nerf_grid_depth_backward";
    int rc = require_grid(fn, grid);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_depth_backward_args);
    GridRenderOpt o{};
    rc = check_grid_options(fn, opt, &o);
    if (rc != NERF_OK) return rc;
    rc = check_rays(fn, a->n_rays, a->origins, a->dirs);
    if (rc != NERF_OK) return rc;
    if (!a->grad_depth && !a->grad_log_transmit) {
        set_error("%s: grad_depth and grad_log_transmit are both NULL: there is nothing to differentiate", fn);
        return NERF_E_INVALID;
    }
    if ((a->grad_depth == nullptr) != (a->tape == nullptr)) {
        set_error("%s: tape must be NULL if and only if grad_depth is NULL", fn);
        return NERF_E_INVALID;
    }
    if (a->n_rays > 0 && !a->grad_density) {
        set_error("%s: grad_density is NULL", fn);
        return NERF_E_INVALID;
    }
    if (a->n_rays == 0) return NERF_OK;
    rc = refuse_palette_grid(fn, grid);      // (the first read of the handle)
    if (rc != NERF_OK) return rc;
    GridDepthBwd r{a->origins, a->dirs, a->n_rays, a->grad_depth, a->grad_log_transmit, a->tape, a->grad_density};
    GridDev g = grid->g;
    g.skip = a->use_skip ? grid->d_skip : nullptr;
    DeviceGuard dg(grid->ctx->device);
    HIP_TRY(launch_grid_depth_bwd(g, o, r, (hipStream_t)a->stream));
    return NERF_OK;
}

}  // extern "C"
