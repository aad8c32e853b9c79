// C ABI of sparse voxel grid resampling (include/nerf_mi355x.h, "Sparse voxel grid: resampling"): argument checks and
// launches. Every check that needs no device comes before the first dereference of a handle and before any launch.
#include <cmath>

#include "compact_device.h"
#include "ctx_internal.h"
#include "grid_internal.h"

using namespace nerf;

extern "C" {

int nerf_grid_lattice_density(nerf_sparse_grid* grid, const nerf_grid_lattice_args* a) {
    const char* fn = "nerf_grid_lattice_density";
    int rc = require_grid(fn, grid);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_lattice_args);
    int64_t n = 0;
    rc = check_grid_reso(fn, a->reso, &n);
    if (rc != NERF_OK) return rc;
    if (!a->xs || !a->ys || !a->zs || !a->density) {
        set_error("%s: xs, ys, zs and density are required", fn);
        return NERF_E_INVALID;
    }
    GridLattice l{};
    l.axis[0] = a->xs;
    l.axis[1] = a->ys;
    l.axis[2] = a->zs;
    for (int k = 0; k < 3; ++k) l.size[k] = a->reso[k];
    l.density = a->density;
    // ---- from here on the handle is read ----
    rc = refuse_palette_grid(fn, grid);
    if (rc != NERF_OK) return rc;
    GridDev g = grid->g;
    g.skip = nullptr;
    DeviceGuard dg(grid->ctx->device);
    HIP_TRY(launch_grid_lattice_density(g, l, (hipStream_t)a->stream));
    return NERF_OK;
}

int nerf_grid_weight_render(nerf_ctx* c, const nerf_grid_camera* cam, const nerf_grid_weight_args* a) {
    const char* fn = "nerf_grid_weight_render";
    int rc = require_ctx(fn, c);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_weight_args);
    GridWeight w{};
    rc = check_grid_camera(fn, cam, &w.cam);
    if (rc != NERF_OK) return rc;
    if (a->last_sample_opaque) {
        set_error("%s: last_sample_opaque is not built", fn);
        return NERF_E_INVALID;
    }
    int64_t n = 0;
    rc = check_grid_reso(fn, a->reso, &n);
    if (rc != NERF_OK) return rc;
    if (!(a->step_size >= 1e-3f) || !std::isfinite(a->step_size) || std::isnan(a->stop_thresh)) {
        set_error("%s: step_size = %g must be finite and >= 1e-3, stop_thresh not NaN", fn, a->step_size);
        return NERF_E_INVALID;
    }
    if (!a->density || !a->max_weight) {
        set_error("%s: density and max_weight are required", fn);
        return NERF_E_INVALID;
    }
    rc = grid_world2grid(fn, a->center, a->radius, a->reso, w.offset, w.scaling);
    if (rc != NERF_OK) return rc;
    for (int k = 0; k < 3; ++k) w.size[k] = a->reso[k];
    w.density = a->density;
    w.max_weight = a->max_weight;
    w.step_size = a->step_size;
    w.stop_thresh = a->stop_thresh;
    DeviceGuard dg(c->device);
    HIP_TRY(launch_grid_weight_render(w, (hipStream_t)a->stream));
    return NERF_OK;
}

int nerf_grid_threshold(nerf_ctx* c, const float* volume, int64_t n, float threshold, uint8_t* mask, void* stream) {
    const char* fn = "nerf_grid_threshold";
    int rc = require_ctx(fn, c);
    if (rc != NERF_OK) return rc;
    if (n < 0 || n > kGridMaxLattice || (n > 0 && (!volume || !mask))) {
        set_error("%s: n = %lld must be in [0, 2^30] and needs volume and mask", fn, (long long)n);
        return NERF_E_INVALID;
    }
    if (std::isnan(threshold)) {
        set_error("%s: threshold is NaN", fn);
        return NERF_E_INVALID;
    }
    DeviceGuard dg(c->device);
    HIP_TRY(launch_grid_threshold(volume, n, threshold, mask, (hipStream_t)stream));
    return NERF_OK;
}

int nerf_grid_dilate(nerf_ctx* c, const int32_t* reso, const uint8_t* in, uint8_t* out, void* stream) {
    const char* fn = "nerf_grid_dilate";
    int rc = require_ctx(fn, c);
    if (rc != NERF_OK) return rc;
    int64_t n = 0;
    rc = check_grid_reso(fn, reso, &n);
    if (rc != NERF_OK) return rc;
    if (!in || !out) {
        set_error("%s: in and out are required", fn);
        return NERF_E_INVALID;
    }
    if (in < out + n && out < in + n) {
        set_error("%s: in and out overlap", fn);
        return NERF_E_INVALID;
    }
    DeviceGuard dg(c->device);
    HIP_TRY(launch_grid_dilate(in, reso, out, (hipStream_t)stream));
    return NERF_OK;
}

int64_t nerf_grid_compact_workspace(int64_t nodes) { return nodes > 0 ? compact_blocks(nodes) : 0; }

int nerf_grid_compact(nerf_ctx* c, const nerf_grid_compact_args* a) {
    const char* fn = "nerf_grid_compact";
    int rc = require_ctx(fn, c);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_compact_args);
    int64_t n = 0;
    rc = check_grid_reso(fn, a->reso, &n);
    if (rc != NERF_OK) return rc;
    if (!a->mask || !a->links || !a->block_offsets || !a->count) {
        set_error("%s: mask, links, block_offsets and count are required", fn);
        return NERF_E_INVALID;
    }
    DeviceGuard dg(c->device);
    HIP_TRY(launch_grid_compact(a->mask, n, a->block_offsets, a->links, a->count, (hipStream_t)a->stream));
    return NERF_OK;
}

int nerf_grid_gather(nerf_sparse_grid* grid, const nerf_grid_gather_args* a) {
    const char* fn = "nerf_grid_gather";
    int rc = require_grid(fn, grid);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_gather_args);
    int64_t n = 0;
    rc = check_grid_reso(fn, a->reso, &n);
    if (rc != NERF_OK) return rc;
    if (a->rows < 0 || a->rows > n) {
        set_error("%s: rows = %lld must be in [0, %lld] (the nodes of the lattice)", fn, (long long)a->rows, (long long)n);
        return NERF_E_INVALID;
    }
    if (a->rows == 0) return NERF_OK;
    if (!a->xs || !a->ys || !a->zs || !a->links || !a->lattice_density || !a->node_of_row || !a->density_data || !a->sh_data) {
        set_error("%s: xs, ys, zs, links, lattice_density, node_of_row, density_data and sh_data are required", fn);
        return NERF_E_INVALID;
    }
    GridGather t{};
    t.axis[0] = a->xs;
    t.axis[1] = a->ys;
    t.axis[2] = a->zs;
    for (int k = 0; k < 3; ++k) t.size[k] = a->reso[k];
    t.links = a->links;
    t.lattice_density = a->lattice_density;
    t.node_of_row = a->node_of_row;
    t.rows = a->rows;
    t.density_data = a->density_data;
    t.sh_data = a->sh_data;
    // ---- from here on the handle is read ----
    rc = refuse_half_grid(fn, grid);
    if (rc != NERF_OK) return rc;
    GridDev g = grid->g;
    g.skip = nullptr;
    DeviceGuard dg(grid->ctx->device);
    HIP_TRY(launch_grid_gather(g, t, (hipStream_t)a->stream));
    return NERF_OK;
}

}  // extern "C"
