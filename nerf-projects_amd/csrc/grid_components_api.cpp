// C ABI of the sparse voxel grid's connected components (include/nerf_mi355x.h, "Sparse voxel grid: connected components"):
// argument checks and launches. Every check that needs no device comes before the first dereference of a handle and before
// any launch.
#include <cmath>

#include "compact_device.h"
#include "ctx_internal.h"
#include "grid_internal.h"

using namespace nerf;

namespace {

int check_count(const char* fn, int64_t n, int64_t count) {
    if (n < 1 || n > kGridMaxLattice || count < 0 || count > n) {
        set_error("%s: n = %lld must be in [1, 2^30] and count = %lld in [0, n]", fn, (long long)n, (long long)count);
        return NERF_E_INVALID;
    }
    return NERF_OK;
}

}  // namespace

extern "C" {

int nerf_grid_components_occupancy(nerf_sparse_grid* grid, const nerf_grid_occupancy_args* a) {
    const char* fn = "nerf_grid_components_occupancy";
    int rc = require_grid(fn, grid);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_occupancy_args);
    if (std::isnan(a->threshold)) {
        set_error("%s: threshold is NaN", fn);
        return NERF_E_INVALID;
    }
    if (!a->occupied) {
        set_error("%s: occupied is required", fn);
        return NERF_E_INVALID;
    }
    // ---- from here on the handle is read ----
    int64_t n = 0;
    rc = check_grid_reso(fn, grid->g.size, &n);
    if (rc != NERF_OK) return rc;
    DeviceGuard dg(grid->ctx->device);
    HIP_TRY(launch_grid_occupancy(grid->g, a->use_density != 0, a->threshold, a->occupied, (hipStream_t)a->stream));
    return NERF_OK;
}

int64_t nerf_grid_components_workspace(int64_t nodes) { return nodes > 0 ? compact_blocks(nodes) : 0; }

int nerf_grid_components_label(nerf_ctx* c, const nerf_grid_label_args* a) {
    const char* fn = "nerf_grid_components_label";
    int rc = require_ctx(fn, c);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_label_args);
    int64_t n = 0;
    rc = check_grid_reso(fn, a->reso, &n);
    if (rc != NERF_OK) return rc;
    if (a->connectivity != 6 && a->connectivity != 18 && a->connectivity != 26) {
        set_error("%s: connectivity = %d must be 6, 18 or 26", fn, a->connectivity);
        return NERF_E_INVALID;
    }
    if (!a->occupied || !a->parent || !a->block_offsets || !a->labels || !a->status) {
        set_error("%s: occupied, parent, block_offsets, labels and status are required", fn);
        return NERF_E_INVALID;
    }
    if (a->parent == a->labels) {
        set_error("%s: parent and labels must be different buffers", fn);
        return NERF_E_INVALID;
    }
    GridLabel l{};
    l.occ = a->occupied;
    for (int k = 0; k < 3; ++k) l.size[k] = a->reso[k];
    l.connectivity = a->connectivity;
    l.parent = a->parent;
    l.block_offsets = a->block_offsets;
    l.labels = a->labels;
    l.status = a->status;
    DeviceGuard dg(c->device);
    HIP_TRY(launch_grid_label(l, (hipStream_t)a->stream));
    return NERF_OK;
}

int nerf_grid_components_finish(nerf_ctx* c, const int32_t* status, int64_t* count, void* stream) {
    const char* fn = "nerf_grid_components_finish";
    int rc = require_ctx(fn, c);
    if (rc != NERF_OK) return rc;
    if (!status || !count) {
        set_error("%s: status and count are required", fn);
        return NERF_E_INVALID;
    }
    DeviceGuard dg(c->device);
    int32_t host[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(host, status, sizeof(host), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (host[1] != 0) {
        set_error("%s: the labelling set its error word to %d (1: a bounded loop hit its cap, 2: a parent it did not write)", fn,
                  host[1]);
        return NERF_E_INTERNAL;
    }
    if (host[0] < 0) {
        set_error("%s: component count %d", fn, host[0]);
        return NERF_E_INTERNAL;
    }
    *count = host[0];
    return NERF_OK;
}

int nerf_grid_components_volumes(nerf_ctx* c, const int32_t* labels, int64_t n, int64_t count, int32_t* volumes, void* stream) {
    const char* fn = "nerf_grid_components_volumes";
    int rc = require_ctx(fn, c);
    if (rc != NERF_OK) return rc;
    rc = check_count(fn, n, count);
    if (rc != NERF_OK) return rc;
    if (count == 0) return NERF_OK;
    if (!labels || !volumes) {
        set_error("%s: labels and volumes are required", fn);
        return NERF_E_INVALID;
    }
    DeviceGuard dg(c->device);
    HIP_TRY(launch_grid_label_volumes(labels, n, count, volumes, (hipStream_t)stream));
    return NERF_OK;
}

int nerf_grid_components_keep(nerf_ctx* c, const int32_t* links, const int32_t* labels, int64_t n, const uint8_t* floater,
                              int64_t count, uint8_t* mask, void* stream) {
    const char* fn = "nerf_grid_components_keep";
    int rc = require_ctx(fn, c);
    if (rc != NERF_OK) return rc;
    rc = check_count(fn, n, count);
    if (rc != NERF_OK) return rc;
    if (!links || !labels || !mask || (count > 0 && !floater)) {
        set_error("%s: links, labels, mask and (with count > 0) floater are required", fn);
        return NERF_E_INVALID;
    }
    DeviceGuard dg(c->device);
    HIP_TRY(launch_grid_keep_mask(links, labels, n, floater, count, mask, (hipStream_t)stream));
    return NERF_OK;
}

int nerf_grid_copy_rows(nerf_ctx* c, const nerf_grid_copy_rows_args* a) {
    const char* fn = "nerf_grid_copy_rows";
    int rc = require_ctx(fn, c);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_copy_rows_args);
    int64_t n = 0;
    rc = check_grid_reso(fn, a->reso, &n);
    if (rc != NERF_OK) return rc;
    if (a->cols < 1 || a->cols > 3 * 9) {
        set_error("%s: cols = %d outside [1, 27]", fn, a->cols);
        return NERF_E_INVALID;
    }
    // old_rows is a grid's capacity, which may exceed the nodes of its lattice (rows no link names); new_rows numbers nodes
    if (a->old_rows < 0 || a->old_rows > 0x7fffffffLL || a->new_rows < 0 || a->new_rows > a->old_rows || a->new_rows > n) {
        set_error("%s: old_rows = %lld must be in [0, 2^31) and new_rows = %lld in [0, min(old_rows, %lld)]", fn,
                  (long long)a->old_rows, (long long)a->new_rows, (long long)n);
        return NERF_E_INVALID;
    }
    if (a->new_rows == 0) return NERF_OK;
    if (!a->old_links || !a->new_links || !a->old_density || !a->old_sh || !a->src_row || !a->density || !a->sh) {
        set_error("%s: old_links, new_links, old_density, old_sh, src_row, density and sh are required", fn);
        return NERF_E_INVALID;
    }
    GridCopyRows r{};
    r.old_links = a->old_links;
    r.new_links = a->new_links;
    r.nodes = n;
    r.old_rows = a->old_rows;
    r.new_rows = a->new_rows;
    r.cols = a->cols;
    r.old_density = a->old_density;
    r.old_sh = a->old_sh;
    r.src_row = a->src_row;
    r.density = a->density;
    r.sh = a->sh;
    DeviceGuard dg(c->device);
    HIP_TRY(launch_grid_copy_rows(r, (hipStream_t)a->stream));
    return NERF_OK;
}

}  // extern "C"
