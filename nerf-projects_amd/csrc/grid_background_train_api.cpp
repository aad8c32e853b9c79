// C ABI of training the sparse voxel grid's background layers (include/nerf_mi355x.h, "Sparse voxel grid: background layers,
// training"): the taped background pass, its backward, the TV gradient and the optimiser step. Every check that needs no
// device comes before the first dereference of a handle and before any launch.
#include <cmath>

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

int require_background(const char* fn, const nerf_sparse_grid* grid) {
    if (grid->bg.links) return NERF_OK;
    set_error("%s: the grid has no background attached (nerf_grid_set_background)", fn);
    return NERF_E_INVALID;
}

constexpr int64_t kBgMaxRows = (int64_t)1 << 35;      // capacity * nlayers: 4 threads each stay inside one launch

}  // namespace

extern "C" {

int nerf_grid_background_rays_taped(nerf_sparse_grid* grid, const nerf_grid_render_options* o,
                                    const nerf_grid_background_taped_args* a) {
    const char* fn = "nerf_grid_background_rays_taped";
    int rc = require_grid(fn, grid);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_background_taped_args);
    GridRenderOpt opt{};
    rc = check_grid_options(fn, o, &opt);
    if (rc != NERF_OK) return rc;
    rc = check_rays(fn, a->n_rays, a->origins, a->dirs);
    if (rc != NERF_OK) return rc;
    if (a->n_rays > 0 && (!a->rgb || !a->log_transmit || !a->log_transmit_out || !a->tape || !a->tape_background)) {
        set_error("%s: rgb, log_transmit, log_transmit_out, tape and tape_background are required", fn);
        return NERF_E_INVALID;
    }
    if (a->n_rays > 0 && a->log_transmit == a->log_transmit_out) {
        set_error("%s: log_transmit_out must be another array than log_transmit (the backward reads the incoming values)", fn);
        return NERF_E_INVALID;
    }
    if (a->n_rays == 0) return NERF_OK;
    // ---- from here on the handle is read ----
    rc = require_background(fn, grid);
    if (rc != NERF_OK) return rc;
    GridBgTaped r{a->origins, a->dirs, a->n_rays, a->rgb, a->log_transmit, a->log_transmit_out, a->tape, a->tape_background};
    GridDev g = grid->g;
    g.skip = nullptr;
    DeviceGuard dg(grid->ctx->device);
    HIP_TRY(launch_grid_background_taped(g, grid->bg, opt, r, (hipStream_t)a->stream));
    return NERF_OK;
}

int nerf_grid_background_backward(nerf_sparse_grid* grid, const nerf_grid_render_options* o,
                                  const nerf_grid_background_backward_args* a) {
    const char* fn = "nerf_grid_background_backward";
    int rc = require_grid(fn, grid);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_background_backward_args);
    GridRenderOpt opt{};
    rc = check_grid_options(fn, o, &opt);
    if (rc != NERF_OK) return rc;
    if (a->sparsity_loss != 0.0f) {
        set_error("%s: sparsity_loss is not built", fn);
        return NERF_E_INVALID;
    }
    if (a->beta_loss != 0.0f) {
        set_error("%s: beta_loss is not built", fn);
        return NERF_E_INVALID;
    }
    rc = check_rays(fn, a->n_rays, a->origins, a->dirs);
    if (rc != NERF_OK) return rc;
    if (a->n_rays > 0 && (!a->grad_rgb || !a->log_transmit || !a->tape_background || !a->grad_background)) {
        set_error("%s: grad_rgb, log_transmit, tape_background and grad_background are required", fn);
        return NERF_E_INVALID;
    }
    if (a->n_rays == 0) return NERF_OK;
    // ---- from here on the handle is read ----
    rc = require_background(fn, grid);
    if (rc != NERF_OK) return rc;
    if (grid->bg.capacity == 0) return NERF_OK;
    GridBgBwd r{a->origins, a->dirs, a->n_rays, a->grad_rgb, a->log_transmit, a->tape_background, a->grad_background,
                a->mask_background};
    GridDev g = grid->g;
    g.skip = nullptr;
    DeviceGuard dg(grid->ctx->device);
    HIP_TRY(launch_grid_background_bwd(g, grid->bg, opt, r, (hipStream_t)a->stream));
    return NERF_OK;
}

int nerf_grid_background_tv_grad(nerf_sparse_grid* grid, const nerf_grid_background_tv_args* a) {
    const char* fn = "nerf_grid_background_tv_grad";
    int rc = require_grid(fn, grid);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_background_tv_args);
    if (!std::isfinite(a->scale_sigma) || !std::isfinite(a->scale_color)) {
        set_error("%s: scale_sigma = %g and scale_color = %g must be finite", fn, a->scale_sigma, a->scale_color);
        return NERF_E_INVALID;
    }
    if (a->count > 0 && (!a->grad || !a->mask)) {
        set_error("%s: grad and mask are required", fn);
        return NERF_E_INVALID;
    }
    // ---- from here on the handle is read ----
    rc = require_background(fn, grid);
    if (rc != NERF_OK) return rc;
    const GridBg& bg = grid->bg;
    const int64_t cells = (int64_t)2 * bg.reso * bg.reso * bg.nlayers;
    if (a->start < 0 || a->start >= cells || a->count < 0 || a->count > cells) {
        set_error("%s: start = %lld must be in [0, %lld) and count = %lld in [0, %lld]", fn, (long long)a->start, (long long)cells,
                  (long long)a->count, (long long)cells);
        return NERF_E_INVALID;
    }
    if (a->count == 0 || bg.capacity == 0) return NERF_OK;
    GridBgTv t{a->start, a->count, a->scale_sigma, a->scale_color, a->grad, a->mask};
    DeviceGuard dg(grid->ctx->device);
    HIP_TRY(launch_grid_background_tv(bg, t, (hipStream_t)a->stream));
    return NERF_OK;
}

int nerf_grid_background_optim_step(nerf_ctx* c, const nerf_grid_background_optim_args* a) {
    const char* fn = "nerf_grid_background_optim_step";
    int rc = require_ctx(fn, c);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_background_optim_args);
    if (a->kind != NERF_GRID_OPTIM_RMSPROP && a->kind != NERF_GRID_OPTIM_SGD) {
        set_error("%s: kind = %d must be NERF_GRID_OPTIM_RMSPROP or NERF_GRID_OPTIM_SGD", fn, a->kind);
        return NERF_E_INVALID;
    }
    if (a->rows < 0 || a->rows > kBgMaxRows) {
        set_error("%s: rows = %lld must be in [0, 2^35]", fn, (long long)a->rows);
        return NERF_E_INVALID;
    }
    if (a->rows > 0 && (!a->data || !a->grad || !a->mask || (a->kind == NERF_GRID_OPTIM_RMSPROP && !a->rms))) {
        set_error("%s: data, grad, mask and (for RMSProp) rms are required", fn);
        return NERF_E_INVALID;
    }
    if (std::isnan(a->lr_sigma) || std::isnan(a->lr_color) || std::isnan(a->minval) ||
        (a->kind == NERF_GRID_OPTIM_RMSPROP && (std::isnan(a->beta) || std::isnan(a->eps)))) {
        set_error("%s: lr_sigma, lr_color, minval, beta and eps must not be NaN", fn);
        return NERF_E_INVALID;
    }
    if (a->rows == 0) return NERF_OK;
    GridBgOptim p{a->data, a->rms, a->grad, a->mask, a->rows, a->beta, a->lr_sigma, a->lr_color, a->eps, a->minval};
    DeviceGuard dg(c->device);
    HIP_TRY(launch_grid_background_optim(p, a->kind == NERF_GRID_OPTIM_RMSPROP, (hipStream_t)a->stream));
    return NERF_OK;
}

}  // extern "C"
