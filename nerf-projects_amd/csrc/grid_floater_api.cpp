// C ABI of the sparse voxel grid's floater views (include/nerf_mi355x.h, "Sparse voxel grid: floater views"): argument checks
// and launches. Every check that needs no device comes before the first dereference of the handle and before any launch.
#include <cmath>

#include "ctx_internal.h"
#include "grid_floater_internal.h"

using namespace nerf;

static_assert(NERF_GRID_FLOATER_COUNTER_INTS == kFloaterCounterSlots * kFloaterSlotStride, "the header's workspace size");

namespace {

// what both calls share: labels, table, the lattice's place in the world, w2c and the camera. The handle is not read.
int check_view(const char* fn, const nerf_grid_camera* cam, const int32_t* labels, const int32_t* table, int64_t n_labels,
               const float radius[3], const float center[3], const float w2c[12], GridFloaterView* v) {
    if (!cam) {
        set_error("%s: nerf_grid_camera is NULL", fn);
        return NERF_E_INVALID;
    }
    GridCam gc{};
    int rc = check_grid_camera(fn, cam, &gc);
    if (rc == NERF_OK) rc = refuse_ndc_camera(fn, gc, "the floater views project world points through a pinhole camera");
    if (rc != NERF_OK) return rc;
    if (!labels || !table) {
        set_error("%s: labels and table are required", fn);
        return NERF_E_INVALID;
    }
    if (n_labels < 0 || n_labels > kGridMaxLattice) {
        set_error("%s: n_labels = %lld must be in [0, 2^30]", fn, (long long)n_labels);
        return NERF_E_INVALID;
    }
    for (int k = 0; k < 3; ++k) {
        if (!(radius[k] > 0.0f) || !std::isfinite(radius[k]) || !std::isfinite(center[k])) {
            set_error("%s: axis %d: radius = %g must be positive and finite, center = %g finite", fn, k, radius[k], center[k]);
            return NERF_E_INVALID;
        }
    }
    for (int i = 0; i < 12; ++i) {
        if (!std::isfinite(w2c[i])) {
            set_error("%s: w2c[%d] = %g is not finite", fn, i, w2c[i]);
            return NERF_E_INVALID;
        }
        v->w2c[i] = w2c[i];
    }
    v->labels = labels;
    v->table = table;
    v->n_labels = n_labels;
    for (int k = 0; k < 3; ++k) {
        v->radius[k] = radius[k];
        v->center[k] = center[k];
    }
    v->fx = (float)gc.fx;
    v->fy = (float)gc.fy;
    v->cx = (float)gc.cx;
    v->cy = (float)gc.cy;
    v->width = gc.width;
    v->height = gc.height;
    return NERF_OK;
}

int read_lattice(const char* fn, const nerf_sparse_grid* grid, GridFloaterView* v) {
    int64_t n = 0;
    const int rc = check_grid_reso(fn, grid->g.size, &n);
    if (rc != NERF_OK) return rc;
    for (int k = 0; k < 3; ++k) v->size[k] = grid->g.size[k];
    v->nodes = n;
    return NERF_OK;
}

}  // namespace

extern "C" {

int nerf_grid_floater_heatmap(nerf_sparse_grid* grid, const nerf_grid_camera* cam, const nerf_grid_floater_heatmap_args* a) {
    const char* fn = "nerf_grid_floater_heatmap";
    int rc = require_grid(fn, grid);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_floater_heatmap_args);
    GridFloaterView v{};
    rc = check_view(fn, cam, a->labels, a->table, a->n_labels, a->radius, a->center, a->w2c, &v);
    if (rc != NERF_OK) return rc;
    if (std::isnan(a->min_density)) {
        set_error("%s: min_density is NaN", fn);
        return NERF_E_INVALID;
    }
    if (a->out_width < 1 || a->out_height < 1 || (int64_t)a->out_width * a->out_height > kGridMaxItems) {
        set_error("%s: heatmap %d x %d must hold between 1 and 2^26 pixels", fn, a->out_width, a->out_height);
        return NERF_E_INVALID;
    }
    if (a->filter_occluded && !a->depth) {
        set_error("%s: filter_occluded needs depth", fn);
        return NERF_E_INVALID;
    }
    if (!a->counts || !a->counters || !a->counter_slots || !a->heatmap) {
        set_error("%s: counts, counters, counter_slots and heatmap are required", fn);
        return NERF_E_INVALID;
    }
    GridFloaterHeat h{};
    h.use_density = a->min_density > 0.0f ? 1 : 0;
    h.min_density = a->min_density;
    h.depth = a->filter_occluded ? a->depth : nullptr;
    h.out_width = a->out_width;
    h.out_height = a->out_height;
    h.counts = a->counts;
    h.counters = a->counters;
    h.counter_slots = a->counter_slots;
    h.heatmap = a->heatmap;
    // ---- from here on the handle is read ----
    rc = read_lattice(fn, grid, &v);
    if (rc != NERF_OK) return rc;
    DeviceGuard dg(grid->ctx->device);
    HIP_TRY(launch_grid_floater_heatmap(grid->g, v, h, (hipStream_t)a->stream));
    return NERF_OK;
}

int nerf_grid_component_view(nerf_sparse_grid* grid, const nerf_grid_camera* cam, const nerf_grid_component_view_args* a) {
    const char* fn = "nerf_grid_component_view";
    int rc = require_grid(fn, grid);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_component_view_args);
    GridFloaterView v{};
    rc = check_view(fn, cam, a->labels, a->table, a->n_labels, a->radius, a->center, a->w2c, &v);
    if (rc != NERF_OK) return rc;
    if (!a->keys || !a->slots) {
        set_error("%s: keys and slots are required", fn);
        return NERF_E_INVALID;
    }
    // ---- from here on the handle is read ----
    rc = read_lattice(fn, grid, &v);
    if (rc != NERF_OK) return rc;
    DeviceGuard dg(grid->ctx->device);
    HIP_TRY(launch_grid_component_view(v, (unsigned long long*)a->keys, a->slots, (hipStream_t)a->stream));
    return NERF_OK;
}

}  // extern "C"
