// C ABI of the sparse voxel grid's gradients for autograd (include/nerf_mi355x.h, "Sparse voxel grid: gradients for
// autograd"): argument checks and launches. Every check that needs no device comes before the first dereference of a handle.
// nerf_grid_render_backward_losses ("Sparse voxel grid: training with the beta and sparsity losses") is nerf_grid_render_backward
// with one more struct, through the same checks.
#include <cmath>

#include "ctx_internal.h"
#include "grid_internal.h"

using namespace nerf;

namespace {

int check_rays(const char* fn, int64_t n_rays) {
    if (n_rays >= 0 && n_rays <= kGridMaxItems) return NERF_OK;
    set_error("%s: n_rays = %lld must be in [0, 2^26]", fn, (long long)n_rays);
    return NERF_E_INVALID;
}

// nerf_grid_render_backward (l == nullptr) and nerf_grid_render_backward_losses
int render_backward(const char* fn, nerf_sparse_grid* grid, const nerf_grid_render_options* o, const nerf_grid_render_backward_args* a,
                    const nerf_grid_render_backward_losses_args* l, bool losses) {
    int rc = require_grid(fn, grid);
    if (rc != NERF_OK) return rc;
    GridRenderOpt opt{};
    rc = check_grid_options(fn, o, &opt);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_render_backward_args);
    if (losses) {
        NERF_CHECK_STRUCT(fn, l, nerf_grid_render_backward_losses_args);
        if (!(std::isfinite(l->beta_loss) && l->beta_loss >= 0.0f)) {
            set_error("%s: beta_loss = %g must be finite and >= 0", fn, l->beta_loss);
            return NERF_E_INVALID;
        }
        if (!(std::isfinite(l->sparsity_loss) && l->sparsity_loss >= 0.0f)) {
            set_error("%s: sparsity_loss = %g must be finite and >= 0", fn, l->sparsity_loss);
            return NERF_E_INVALID;
        }
    }
    rc = check_rays(fn, a->n_rays);
    if (rc != NERF_OK) return rc;
    if (a->n_rays > 0 && (!a->origins || !a->dirs || !a->grad_rgb || !a->tape)) {
        set_error("%s: origins, dirs, grad_rgb and tape are required", fn);
        return NERF_E_INVALID;
    }
    const bool terms = losses && (l->beta_loss > 0.0f || l->sparsity_loss > 0.0f);
    if (a->n_rays > 0 && terms) {
        if (l->beta_loss > 0.0f && !l->log_transmit) {
            set_error("%s: log_transmit is required with beta_loss > 0", fn);
            return NERF_E_INVALID;
        }
        if (!a->grad_density) {
            set_error("%s: grad_density is required with beta_loss > 0 or sparsity_loss > 0 (the terms are density gradients)", fn);
            return NERF_E_INVALID;
        }
    }
    if (a->n_rays == 0 || (!a->grad_density && !a->grad_sh && !a->mask)) return NERF_OK;
    GridRenderBwd r{a->origins, a->dirs, a->n_rays, a->grad_rgb, a->tape, a->grad_density, a->grad_sh, a->mask};
    if (terms) {
        r.log_transmit = l->log_transmit;
        r.beta_loss = l->beta_loss;
        r.sparsity_loss = l->sparsity_loss;
    }
    rc = refuse_half_grid(fn, grid);      // (the first read of the handle)
    if (rc != NERF_OK) return rc;
    GridDev g = grid->g;
    g.skip = a->use_skip ? grid->d_skip : nullptr;
    DeviceGuard dg(grid->ctx->device);
    // with both weights 0 the losses entry is the plain one: the same kernel
    if (terms)
        HIP_TRY(launch_grid_render_bwd_losses(g, opt, r, (hipStream_t)a->stream));
    else
        HIP_TRY(launch_grid_render_bwd(g, opt, r, (hipStream_t)a->stream));
    return NERF_OK;
}

}  // namespace

extern "C" {

int nerf_grid_render_rays_taped(nerf_sparse_grid* grid, const nerf_grid_render_options* o, const nerf_grid_render_taped_args* a) {
    const char* fn = "nerf_grid_render_rays_taped";
    int rc = require_grid(fn, grid);
    if (rc != NERF_OK) return rc;
    GridRenderOpt opt{};
    rc = check_grid_options(fn, o, &opt);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_render_taped_args);
    rc = check_rays(fn, a->n_rays);
    if (rc != NERF_OK) return rc;
    if (a->n_rays > 0 && (!a->origins || !a->dirs || !a->rgb_out || !a->tape)) {
        set_error("%s: origins, dirs, rgb_out and tape are required", fn);
        return NERF_E_INVALID;
    }
    if (a->n_rays == 0) return NERF_OK;
    GridTaped r{a->origins, a->dirs, a->n_rays, a->rgb_out, a->log_transmit, a->tape};
    rc = refuse_half_grid(fn, grid);      // (the first read of the handle)
    if (rc != NERF_OK) return rc;
    GridDev g = grid->g;
    g.skip = a->use_skip ? grid->d_skip : nullptr;
    DeviceGuard dg(grid->ctx->device);
    HIP_TRY(launch_grid_render_taped(g, opt, r, (hipStream_t)a->stream));
    return NERF_OK;
}

int nerf_grid_render_backward(nerf_sparse_grid* grid, const nerf_grid_render_options* o, const nerf_grid_render_backward_args* a) {
    return render_backward("nerf_grid_render_backward", grid, o, a, nullptr, false);
}

int nerf_grid_render_backward_losses(nerf_sparse_grid* grid, const nerf_grid_render_options* o, const nerf_grid_render_backward_args* a,
                                     const nerf_grid_render_backward_losses_args* l) {
    return render_backward("nerf_grid_render_backward_losses", grid, o, a, l, true);
}

int nerf_grid_sample_backward(nerf_sparse_grid* grid, const nerf_grid_sample_backward_args* a) {
    const char* fn = "nerf_grid_sample_backward";
    int rc = require_grid(fn, grid);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_sample_backward_args);
    if (a->n < 0 || a->n > kGridMaxItems) {
        set_error("%s: n = %lld must be in [0, 2^26]", fn, (long long)a->n);
        return NERF_E_INVALID;
    }
    if (a->n > 0 && (!a->points || !a->grad_out_density || (a->want_colors && a->grad_sh && !a->grad_out_sh))) {
        set_error("%s: points, grad_out_density and (with want_colors and grad_sh) grad_out_sh are required", fn);
        return NERF_E_INVALID;
    }
    if (a->n == 0 || (!a->grad_density && !(a->want_colors && a->grad_sh))) return NERF_OK;
    GridSampleBwd p{a->points, a->n, a->grid_coords, a->want_colors, a->grad_out_density, a->grad_out_sh, a->grad_density,
                    a->grad_sh};
    rc = refuse_half_grid(fn, grid);      // (the first read of the handle)
    if (rc != NERF_OK) return rc;
    DeviceGuard dg(grid->ctx->device);
    HIP_TRY(launch_grid_sample_bwd(grid->g, p, (hipStream_t)a->stream));
    return NERF_OK;
}

}  // extern "C"
