// C ABI of sparse voxel grid training (include/nerf_mi355x.h, "Sparse voxel grid: training" and "Sparse voxel grid: training
// with the beta and sparsity losses"): argument checks and launches. Every check that needs no device comes before the first
// dereference of a handle. nerf_grid_fused_backward / nerf_grid_fused_backward_losses and nerf_grid_tv_grad /
// nerf_grid_tv_grad_edge share one set of checks each: the older entry of a pair refuses what only the newer one has built.
#include <cmath>

#include "ctx_internal.h"
#include "grid_internal.h"

using namespace nerf;

namespace {

// a loss weight of the *_losses entries: finite and >= 0
int check_loss_weight(const char* fn, const char* field, float v) {
    if (std::isfinite(v) && v >= 0.0f) return NERF_OK;
    set_error("%s: %s = %g must be finite and >= 0", fn, field, v);
    return NERF_E_INVALID;
}

int fused_backward(const char* fn, bool losses, nerf_sparse_grid* grid, const nerf_grid_render_options* o, const nerf_grid_fused_args* a) {
    int rc = require_grid(fn, grid);
    if (rc != NERF_OK) return rc;
    GridRenderOpt opt{};
    rc = check_grid_options(fn, o, &opt);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_fused_args);
    if (losses) {
        rc = check_loss_weight(fn, "beta_loss", a->beta_loss);
        if (rc == NERF_OK) rc = check_loss_weight(fn, "sparsity_loss", a->sparsity_loss);
        if (rc != NERF_OK) return rc;
    } else if (a->beta_loss != 0.0f) {
        set_error("%s: beta_loss is not built here: nerf_grid_fused_backward_losses has it", fn);
        return NERF_E_INVALID;
    } else if (a->sparsity_loss != 0.0f) {
        set_error("%s: sparsity_loss is not built here: nerf_grid_fused_backward_losses has it", fn);
        return NERF_E_INVALID;
    }
    if (a->background_nlayers != 0) {
        set_error("%s: background layers are not built", fn);
        return NERF_E_INVALID;
    }
    if (a->n_rays < 0 || a->n_rays > kGridMaxItems) {
        set_error("%s: n_rays = %lld must be in [0, 2^26]", fn, (long long)a->n_rays);
        return NERF_E_INVALID;
    }
    if (a->n_rays > 0 && (!a->origins || !a->dirs || !a->rgb_gt || !a->rgb_out || !a->grad_density || !a->grad_sh || !a->mask)) {
        set_error("%s: origins, dirs, rgb_gt, rgb_out, grad_density, grad_sh and mask are required", fn);
        return NERF_E_INVALID;
    }
    if (a->n_rays == 0) return NERF_OK;
    GridFused r{};
    r.origins = a->origins;
    r.dirs = a->dirs;
    r.rgb_gt = a->rgb_gt;
    r.n_rays = a->n_rays;
    r.grad_scale = 2.0f / (3.0f * (float)a->n_rays);
    r.rgb = a->rgb_out;
    r.log_transmit = a->log_transmit;
    r.grad_density = a->grad_density;
    r.grad_sh = a->grad_sh;
    r.mask = a->mask;
    r.beta_loss = a->beta_loss;
    r.sparsity_loss = a->sparsity_loss;
    rc = refuse_half_grid(fn, grid);      // (the first read of the handle)
    if (rc != NERF_OK) return rc;
    GridDev g = grid->g;
    g.skip = a->use_skip ? grid->d_skip : nullptr;
    DeviceGuard dg(grid->ctx->device);
    // with both weights 0 the losses entry is the plain one: the same kernel
    if (r.beta_loss > 0.0f || r.sparsity_loss > 0.0f)
        HIP_TRY(launch_grid_fused_losses(g, opt, r, (hipStream_t)a->stream));
    else
        HIP_TRY(launch_grid_fused(g, opt, r, (hipStream_t)a->stream));
    return NERF_OK;
}

int tv_grad(const char* fn, bool edge_entry, nerf_sparse_grid* grid, const nerf_grid_tv_args* a) {
    int rc = require_grid(fn, grid);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_tv_args);
    if (edge_entry) {
        if (a->ignore_edge != 0 && a->ignore_edge != 1) {
            set_error("%s: ignore_edge = %d must be 0 or 1", fn, a->ignore_edge);
            return NERF_E_INVALID;
        }
        if (a->ignore_last_z || a->use_ndc) {
            set_error("%s: ignore_last_z and NDC scaling are not built", fn);
            return NERF_E_INVALID;
        }
    } else if (a->ignore_edge || a->ignore_last_z || a->use_ndc) {
        set_error("%s: ignore_edge, ignore_last_z and NDC scaling are not built here: nerf_grid_tv_grad_edge has ignore_edge", fn);
        return NERF_E_INVALID;
    }
    if (a->target != NERF_GRID_TV_DENSITY && a->target != NERF_GRID_TV_SH) {
        set_error("%s: target = %d must be NERF_GRID_TV_DENSITY or NERF_GRID_TV_SH", fn, a->target);
        return NERF_E_INVALID;
    }
    if (!std::isfinite(a->scale)) {
        set_error("%s: scale = %g must be finite", fn, a->scale);
        return NERF_E_INVALID;
    }
    if (a->count > 0 && (!a->grad || !a->mask)) {
        set_error("%s: grad and mask are required", fn);
        return NERF_E_INVALID;
    }
    // ---- from here on the handle is read ----
    rc = refuse_palette_grid(fn, grid);
    if (rc != NERF_OK) return rc;
    if (a->target == NERF_GRID_TV_SH) {
        rc = refuse_half_grid(fn, grid);
        if (rc != NERF_OK) return rc;
    }
    const GridDev& g = grid->g;
    const int64_t n = (int64_t)g.size[0] * g.size[1] * g.size[2];
    const int cols = a->target == NERF_GRID_TV_DENSITY ? 1 : 3 * g.basis_dim;
    if (a->start < 0 || a->start >= n || a->count < 0 || a->count > n) {
        set_error("%s: start = %lld must be in [0, %lld) and count = %lld in [0, %lld]", fn, (long long)a->start, (long long)n,
                  (long long)a->count, (long long)n);
        return NERF_E_INVALID;
    }
    if (a->start_dim < 0 || a->end_dim > cols || a->start_dim > a->end_dim) {
        set_error("%s: columns [%d, %d) outside [0, %d)", fn, a->start_dim, a->end_dim, cols);
        return NERF_E_INVALID;
    }
    if (a->count == 0 || a->start_dim == a->end_dim || g.capacity == 0) return NERF_OK;
    GridTv t{};
    t.data = a->target == NERF_GRID_TV_DENSITY ? g.density : g.sh;
    t.grad = a->grad;
    t.mask = a->mask;
    t.start = a->start;
    t.count = a->count;
    t.cols = cols;
    t.start_dim = a->start_dim;
    t.end_dim = a->end_dim;
    t.scale = a->scale;
    for (int k = 0; k < 3; ++k) t.axis_scale[k] = (float)g.size[k] * (1.0f / 256.0f);
    DeviceGuard dg(grid->ctx->device);
    if (a->ignore_edge)
        HIP_TRY(launch_grid_tv_grad_edge(g, t, (hipStream_t)a->stream));
    else
        HIP_TRY(launch_grid_tv_grad(g, t, (hipStream_t)a->stream));
    return NERF_OK;
}

}  // namespace

extern "C" {

int nerf_grid_fused_backward(nerf_sparse_grid* grid, const nerf_grid_render_options* o, const nerf_grid_fused_args* a) {
    return fused_backward("nerf_grid_fused_backward", false, grid, o, a);
}

int nerf_grid_fused_backward_losses(nerf_sparse_grid* grid, const nerf_grid_render_options* o, const nerf_grid_fused_args* a) {
    return fused_backward("nerf_grid_fused_backward_losses", true, grid, o, a);
}

int nerf_grid_tv_grad(nerf_sparse_grid* grid, const nerf_grid_tv_args* a) { return tv_grad("nerf_grid_tv_grad", false, grid, a); }

int nerf_grid_tv_grad_edge(nerf_sparse_grid* grid, const nerf_grid_tv_args* a) { return tv_grad("nerf_grid_tv_grad_edge", true, grid, a); }

int nerf_grid_optim_step(nerf_ctx* c, const nerf_grid_optim_args* a) {
    const char* fn = "nerf_grid_optim_step";
    int rc = require_ctx(fn, c);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_optim_args);
    if (a->kind != NERF_GRID_OPTIM_RMSPROP && a->kind != NERF_GRID_OPTIM_SGD) {
        set_error("%s: kind = %d must be NERF_GRID_OPTIM_RMSPROP or NERF_GRID_OPTIM_SGD", fn, a->kind);
        return NERF_E_INVALID;
    }
    if (a->rows < 0 || a->rows > 0x7fffffffLL || a->cols < 1 || a->cols > 4096) {
        set_error("%s: rows = %lld must be in [0, 2^31) and cols = %d in [1, 4096]", fn, (long long)a->rows, a->cols);
        return NERF_E_INVALID;
    }
    if (a->rows > 0 && (!a->data || !a->grad || !a->mask || (a->kind == NERF_GRID_OPTIM_RMSPROP && !a->rms))) {
        set_error("%s: data, grad, mask and (for RMSProp) rms are required", fn);
        return NERF_E_INVALID;
    }
    if (std::isnan(a->lr) || std::isnan(a->minval) || (a->kind == NERF_GRID_OPTIM_RMSPROP && (std::isnan(a->beta) || std::isnan(a->eps)))) {
        set_error("%s: lr, minval, beta and eps must not be NaN", fn);
        return NERF_E_INVALID;
    }
    if (a->rows == 0) return NERF_OK;
    GridOptim p{a->data, a->rms, a->grad, a->mask, a->rows, a->cols, a->beta, a->lr, a->eps, a->minval};
    DeviceGuard dg(c->device);
    HIP_TRY(launch_grid_optim_step(p, a->kind == NERF_GRID_OPTIM_RMSPROP, (hipStream_t)a->stream));
    return NERF_OK;
}

}  // extern "C"
