// C ABI of the sparse voxel grid's regularisers as values (include/nerf_mi355x.h, "Sparse voxel grid: regularisers as
// values"): argument checks and the launches. Every check that needs no device comes before the first dereference of the
// handle and before any launch. The value and its backward share one set of checks each.
#include "ctx_internal.h"
#include "grid_internal.h"

using namespace nerf;

namespace {

int tv_value(const char* fn, bool backward, nerf_sparse_grid* grid, const nerf_grid_tv_value_args* a) {
    int rc = require_grid(fn, grid);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_tv_value_args);
    if (a->target != NERF_GRID_TV_DENSITY && a->target != NERF_GRID_TV_SH) {
        set_error("%s: target = %d must be NERF_GRID_TV_DENSITY or NERF_GRID_TV_SH", fn, a->target);
        return NERF_E_INVALID;
    }
    if (a->ignore_edge != 0 && a->ignore_edge != 1) {
        set_error("%s: ignore_edge = %d must be 0 or 1", fn, a->ignore_edge);
        return NERF_E_INVALID;
    }
    if (a->cells && (a->cells_int64 != 0 && a->cells_int64 != 1)) {
        set_error("%s: cells_int64 = %d must be 0 or 1", fn, a->cells_int64);
        return NERF_E_INVALID;
    }
    if (a->cells && (a->n_cells < 0 || a->n_cells > kGridMaxLattice)) {
        set_error("%s: n_cells = %lld must be in [0, 2^30]", fn, (long long)a->n_cells);
        return NERF_E_INVALID;
    }
    // (the density has one column; how many the SH table has is known only from the handle, below)
    if (a->start_dim < 0 || a->start_dim > a->end_dim || (a->target == NERF_GRID_TV_DENSITY && a->end_dim > 1)) {
        set_error("%s: columns [%d, %d) outside the table", fn, a->start_dim, a->end_dim);
        return NERF_E_INVALID;
    }
    if (backward) {
        if (!a->grad_value || !a->grad) {
            set_error("%s: grad_value and grad are required", fn);
            return NERF_E_INVALID;
        }
    } else if (!a->value) {
        set_error("%s: value is NULL", fn);
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
    const int cols = a->target == NERF_GRID_TV_DENSITY ? 1 : 3 * g.basis_dim;
    if (a->end_dim > cols) {
        set_error("%s: columns [%d, %d) outside [0, %d)", fn, a->start_dim, a->end_dim, cols);
        return NERF_E_INVALID;
    }
    GridTvValue t{};
    t.data = a->target == NERF_GRID_TV_DENSITY ? g.density : g.sh;
    t.cols = cols;
    t.start_dim = a->start_dim;
    t.end_dim = a->end_dim;
    t.edge = a->ignore_edge;
    t.cells = a->cells;
    t.cells_int64 = a->cells_int64;
    t.count = a->cells ? a->n_cells : (int64_t)(g.size[0] - 1) * (g.size[1] - 1) * (g.size[2] - 1);
    for (int k = 0; k < 3; ++k) t.axis_scale[k] = (float)g.size[k] * (1.0f / 256.0f);
    t.partials = a->partials;
    t.value = a->value;
    t.grad_value = a->grad_value;
    t.grad = a->grad;
    if (!backward && t.count * (t.end_dim - t.start_dim) > 0 && !a->partials) {
        set_error("%s: partials is NULL", fn);
        return NERF_E_INVALID;
    }
    DeviceGuard dg(grid->ctx->device);
    if (backward)
        HIP_TRY(launch_grid_tv_value_bwd(g, t, (hipStream_t)a->stream));
    else
        HIP_TRY(launch_grid_tv_value(g, t, (hipStream_t)a->stream));
    return NERF_OK;
}

int sparsity(const char* fn, bool backward, nerf_sparse_grid* grid, const nerf_grid_render_options* opt, const nerf_grid_sparsity_args* a) {
    int rc = require_grid(fn, grid);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_sparsity_args);
    GridRenderOpt o{};
    rc = check_grid_options(fn, opt, &o);
    if (rc != NERF_OK) return rc;
    if (a->n_rays < 0 || a->n_rays > kGridMaxItems || (a->n_rays > 0 && (!a->origins || !a->dirs))) {
        set_error("%s: n_rays = %lld must be in [0, 2^26] and needs origins and dirs", fn, (long long)a->n_rays);
        return NERF_E_INVALID;
    }
    if (a->n_rays > 0 && backward && (!a->grad_sparsity || !a->grad_density)) {
        set_error("%s: grad_sparsity and grad_density are required", fn);
        return NERF_E_INVALID;
    }
    if (a->n_rays > 0 && !backward && !a->sparsity) {
        set_error("%s: sparsity is NULL", fn);
        return NERF_E_INVALID;
    }
    if (a->n_rays == 0) return NERF_OK;
    rc = refuse_palette_grid(fn, grid);      // (the first read of the handle)
    if (rc != NERF_OK) return rc;
    GridSparsity r{a->origins, a->dirs, a->n_rays, a->sparsity, a->grad_sparsity, a->grad_density};
    GridDev g = grid->g;
    g.skip = a->use_skip ? grid->d_skip : nullptr;
    DeviceGuard dg(grid->ctx->device);
    if (backward)
        HIP_TRY(launch_grid_sparsity_bwd(g, o, r, (hipStream_t)a->stream));
    else
        HIP_TRY(launch_grid_sparsity(g, o, r, (hipStream_t)a->stream));
    return NERF_OK;
}

}  // namespace

extern "C" {

int64_t nerf_grid_tv_value_workspace(int64_t items) {
    return items > 0 ? (items + kGridTvValueItems - 1) / kGridTvValueItems : 0;
}

int nerf_grid_tv_value(nerf_sparse_grid* grid, const nerf_grid_tv_value_args* a) { return tv_value("nerf_grid_tv_value", false, grid, a); }

int nerf_grid_tv_value_backward(nerf_sparse_grid* grid, const nerf_grid_tv_value_args* a) {
    return tv_value("nerf_grid_tv_value_backward", true, grid, a);
}

int nerf_grid_sparsity_rays(nerf_sparse_grid* grid, const nerf_grid_render_options* opt, const nerf_grid_sparsity_args* a) {
    return sparsity("nerf_grid_sparsity_rays", false, grid, opt, a);
}

int nerf_grid_sparsity_backward(nerf_sparse_grid* grid, const nerf_grid_render_options* opt, const nerf_grid_sparsity_args* a) {
    return sparsity("nerf_grid_sparsity_backward", true, grid, opt, a);
}

}  // extern "C"
