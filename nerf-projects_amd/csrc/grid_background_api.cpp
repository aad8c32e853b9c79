// C ABI of the sparse voxel grid's background layers (include/nerf_mi355x.h, "Sparse voxel grid: background layers"): attach /
// detach, the background pass over rays or a camera, and the two calls of the thinning. Every check that needs no device
// comes before the first dereference of a handle and before any launch.
#include <cmath>

#include "ctx_internal.h"
#include "grid_internal.h"

using namespace nerf;

namespace {

constexpr int kBgMaxLayers = 1024;
constexpr int kBgMaxDilate = 64;

// nlayers, reso, capacity and the two tables of a background: what the desc and the thinning calls have in common
int check_background_shape(const char* fn, int32_t nlayers, int32_t reso, int64_t capacity, const int32_t* links, const float* data,
                           GridBg* out) {
    if (nlayers < 2 || nlayers > kBgMaxLayers) {
        set_error("%s: nlayers = %d outside [2, %d]", fn, nlayers, kBgMaxLayers);
        return NERF_E_INVALID;
    }
    if (reso < 2 || reso > 1024) {
        set_error("%s: reso = %d outside [2, 1024]", fn, reso);
        return NERF_E_INVALID;
    }
    if (capacity < 0 || capacity > 0x7fffffffLL || !links || (capacity > 0 && !data)) {
        set_error("%s: links, and with capacity = %lld > 0 (below 2^31) data, are required", fn, (long long)capacity);
        return NERF_E_INVALID;
    }
    if ((uintptr_t)data & 15) {
        set_error("%s: data is not 16-byte aligned", fn);
        return NERF_E_INVALID;
    }
    *out = GridBg{links, data, nlayers, reso, capacity};
    return NERF_OK;
}

int background(const char* fn, nerf_sparse_grid* grid, const nerf_grid_camera* cam, const nerf_grid_render_options* opt,
               const nerf_grid_background_args* a) {
    int rc = require_grid(fn, grid);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_background_args);
    GridRenderOpt o{};
    rc = check_grid_options(fn, opt, &o);
    if (rc != NERF_OK) return rc;
    GridBgRender r{};
    if (cam) {
        rc = check_grid_camera(fn, cam, &r.cam);
        if (rc == NERF_OK) rc = refuse_ndc_camera(fn, r.cam, "background layers are for unbounded scenes, which svox2 never combines with NDC");
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
    if (r.n_rays > 0 && (!a->rgb || !a->log_transmit)) {
        set_error("%s: rgb and log_transmit (both in / out) are required", fn);
        return NERF_E_INVALID;
    }
    if (r.n_rays == 0) return NERF_OK;
    r.rgb = a->rgb;
    r.log_transmit = a->log_transmit;
    // ---- from here on the handle is read ----
    if (!grid->bg.links) {
        set_error("%s: the grid has no background attached (nerf_grid_set_background)", fn);
        return NERF_E_INVALID;
    }
    GridDev g = grid->g;
    g.skip = nullptr;
    DeviceGuard dg(grid->ctx->device);
    HIP_TRY(launch_grid_background(g, grid->bg, o, r, (hipStream_t)a->stream));
    return NERF_OK;
}

}  // namespace

extern "C" {

int nerf_grid_set_background(nerf_sparse_grid* grid, const nerf_grid_background_desc* d) {
    const char* fn = "nerf_grid_set_background";
    int rc = require_grid(fn, grid);
    if (rc != NERF_OK) return rc;
    GridBg bg{};
    if (d) {
        NERF_CHECK_STRUCT(fn, d, nerf_grid_background_desc);
        rc = check_background_shape(fn, d->nlayers, d->reso, d->capacity, d->links, d->data, &bg);
        if (rc != NERF_OK) return rc;
    }
    // ---- from here on the handle is read ----
    if (!d) {
        grid->bg = GridBg{};
        return NERF_OK;
    }
    if (grid->half) {
        set_error("%s: a half-precision grid (nerf_grid_create_half) takes no background: attach it to a grid of nerf_grid_create", fn);
        return NERF_E_INVALID;
    }
    if (grid->palette) {
        set_error("%s: a palette grid (nerf_grid_create_palette) takes no background: attach it to a grid of nerf_grid_create", fn);
        return NERF_E_INVALID;
    }
    DeviceGuard dg(grid->ctx->device);
    rc = check_grid_links(fn, d->links, (int64_t)2 * d->reso * d->reso, d->capacity, (hipStream_t)d->stream);
    if (rc != NERF_OK) return rc;
    grid->bg = bg;
    return NERF_OK;
}

int nerf_grid_has_background(const nerf_sparse_grid* grid) { return grid && grid->bg.links ? 1 : 0; }

int nerf_grid_background_rays(nerf_sparse_grid* grid, const nerf_grid_render_options* opt, const nerf_grid_background_args* args) {
    return background("nerf_grid_background_rays", grid, nullptr, opt, args);
}

int nerf_grid_background_image(nerf_sparse_grid* grid, const nerf_grid_camera* cam, const nerf_grid_render_options* opt,
                               const nerf_grid_background_args* args) {
    if (!cam) {
        set_error("nerf_grid_background_image: nerf_grid_camera is NULL");
        return NERF_E_INVALID;
    }
    return background("nerf_grid_background_image", grid, cam, opt, args);
}

int nerf_grid_background_sparsify_plan(nerf_ctx* c, const nerf_grid_background_sparsify_args* a) {
    const char* fn = "nerf_grid_background_sparsify_plan";
    int rc = require_ctx(fn, c);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_background_sparsify_args);
    GridBgSparsify p{};
    rc = check_background_shape(fn, a->nlayers, a->reso, a->capacity, a->links, a->data, &p.bg);
    if (rc != NERF_OK) return rc;
    if ((int64_t)2 * a->reso * a->reso * a->nlayers > kGridMaxLattice) {
        set_error("%s: 2 reso^2 nlayers = %lld mask entries, at most 2^30", fn, (long long)2 * a->reso * a->reso * a->nlayers);
        return NERF_E_INVALID;
    }
    if (std::isnan(a->sigma_thresh) || a->dilate < 0 || a->dilate > kBgMaxDilate) {
        set_error("%s: sigma_thresh must not be NaN and dilate = %d lie in [0, %d]", fn, a->dilate, kBgMaxDilate);
        return NERF_E_INVALID;
    }
    if (!a->mask || !a->keep || !a->block_offsets || !a->new_links || !a->count) {
        set_error("%s: mask, keep, block_offsets, new_links and count are required", fn);
        return NERF_E_INVALID;
    }
    p.sigma_thresh = a->sigma_thresh;
    p.dilate = a->dilate;
    p.mask = a->mask;
    p.keep = a->keep;
    p.block_offsets = a->block_offsets;
    p.new_links = a->new_links;
    p.count = a->count;
    DeviceGuard dg(c->device);
    HIP_TRY(launch_grid_background_plan(p, (hipStream_t)a->stream));
    return NERF_OK;
}

int nerf_grid_background_gather(nerf_ctx* c, const nerf_grid_background_gather_args* a) {
    const char* fn = "nerf_grid_background_gather";
    int rc = require_ctx(fn, c);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_background_gather_args);
    GridBg bg{};
    rc = check_background_shape(fn, a->nlayers, a->reso, a->capacity, a->links, a->data, &bg);
    if (rc != NERF_OK) return rc;
    const int64_t texels = (int64_t)2 * a->reso * a->reso;
    if (a->new_capacity < 0 || a->new_capacity > texels || a->new_capacity > a->capacity) {
        set_error("%s: new_capacity = %lld must be in [0, min(capacity, 2 reso^2)]", fn, (long long)a->new_capacity);
        return NERF_E_INVALID;
    }
    if (a->new_capacity == 0) return NERF_OK;
    if (!a->new_links || !a->new_data || ((uintptr_t)a->new_data & 15)) {
        set_error("%s: new_links and new_data (16-byte aligned) are required", fn);
        return NERF_E_INVALID;
    }
    const int64_t row = (int64_t)a->nlayers * 4;
    if (a->new_data < a->data + a->capacity * row && a->data < a->new_data + a->new_capacity * row) {
        set_error("%s: data and new_data overlap", fn);
        return NERF_E_INVALID;
    }
    DeviceGuard dg(c->device);
    HIP_TRY(launch_grid_background_gather(bg, a->new_links, a->new_capacity, a->new_data, (hipStream_t)a->stream));
    return NERF_OK;
}

}  // extern "C"
