// C ABI of the sparse voxel grid's surface meshes (include/nerf_mi355x.h, "Sparse voxel grid: surface meshes"): argument
// checks and launches. Every check that needs no device comes before the first dereference of a handle and before any launch.
#include <cmath>

#include "ctx_internal.h"
#include "grid_internal.h"
#include "nerf_internal.h"

using namespace nerf;

extern "C" {

int nerf_grid_marching_cubes(nerf_sparse_grid* grid, const nerf_grid_mc_args* a) {
    const char* fn = "nerf_grid_marching_cubes";
    int rc = require_grid(fn, grid);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_mc_args);
    if (!(a->iso > 0.0f) || !std::isfinite(a->iso)) {
        set_error("%s: iso = %g must be finite and > 0 (an empty node has the value 0 and is outside)", fn, a->iso);
        return NERF_E_INVALID;
    }
    if (!a->n_vertices || !a->n_triangles) {
        set_error("%s: n_vertices and n_triangles are required", fn);
        return NERF_E_INVALID;
    }
    const bool count_only = !a->vertices && !a->triangles;
    if (!count_only && (!a->vertices || !a->triangles)) {
        set_error("%s: vertices and triangles must both be given, or both be NULL (count only)", fn);
        return NERF_E_INVALID;
    }
    if (!count_only && (a->vertex_capacity < 0 || a->triangle_capacity < 0)) {
        set_error("%s: negative capacity", fn);
        return NERF_E_INVALID;
    }
    // ---- from here on the handle is read ----
    int64_t nodes = 0;
    rc = check_grid_reso(fn, grid->g.size, &nodes);
    if (rc != NERF_OK) return rc;
    nerf_ctx* c = grid->ctx;
    DeviceGuard dg(c->device);
    hipStream_t s = (hipStream_t)a->stream;
    ScratchScope scope(c, s);
    HIP_TRY(scope.status);
    rc = ensure_workspace(c, mc_scratch_bytes(grid->g.size));
    if (rc != NERF_OK) return rc;
    McGridArgs m{grid->g.links, grid->g.density, a->mask, grid->g.capacity, {grid->g.size[0], grid->g.size[1], grid->g.size[2]},
                 a->iso, a->vertices, a->triangles};
    int64_t totals[2] = {0, 0};
    HIP_TRY(launch_grid_mc_count(m, c->ws, totals, s));
    *a->n_vertices = totals[0];
    *a->n_triangles = totals[1];
    if (count_only) return NERF_OK;
    if (totals[0] > a->vertex_capacity || totals[1] > a->triangle_capacity) {
        set_error("%s: the mesh has %lld vertices and %lld triangles; capacities %lld and %lld (nothing was written)", fn,
                  (long long)totals[0], (long long)totals[1], (long long)a->vertex_capacity, (long long)a->triangle_capacity);
        return NERF_E_INVALID;
    }
    HIP_TRY(launch_grid_mc_emit(m, c->ws, s));
    return NERF_OK;
}

int nerf_grid_mesh_attributes(nerf_sparse_grid* grid, const nerf_grid_mesh_attributes_args* a) {
    const char* fn = "nerf_grid_mesh_attributes";
    int rc = require_grid(fn, grid);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_mesh_attributes_args);
    if (a->n < 0 || a->n > kGridMaxItems || (a->n > 0 && !a->points)) {
        set_error("%s: n = %lld must be in [0, 2^26] and needs points", fn, (long long)a->n);
        return NERF_E_INVALID;
    }
    if (a->color_mode < NERF_GRID_MESH_COLOR_NONE || a->color_mode > NERF_GRID_MESH_COLOR_VIEW) {
        set_error("%s: color_mode = %d is not one of NERF_GRID_MESH_COLOR_*", fn, a->color_mode);
        return NERF_E_INVALID;
    }
    if ((a->color_mode != NERF_GRID_MESH_COLOR_NONE) != (a->colors != nullptr)) {
        set_error("%s: colors must be given with a colour mode and be NULL with NERF_GRID_MESH_COLOR_NONE", fn);
        return NERF_E_INVALID;
    }
    if (!a->normals && !a->colors) {
        set_error("%s: nothing to compute: normals and colors are both NULL", fn);
        return NERF_E_INVALID;
    }
    if (a->color_mode == NERF_GRID_MESH_COLOR_VIEW) {
        const double n2 = (double)a->view[0] * a->view[0] + (double)a->view[1] * a->view[1] + (double)a->view[2] * a->view[2];
        if (!(std::fabs(n2 - 1.0) <= 1e-5)) {
            set_error("%s: view = (%g, %g, %g) must be a unit vector", fn, a->view[0], a->view[1], a->view[2]);
            return NERF_E_INVALID;
        }
    }
    // ---- from here on the handle is read ----
    int64_t nodes = 0;
    rc = check_grid_reso(fn, grid->g.size, &nodes);
    if (rc != NERF_OK) return rc;
    DeviceGuard dg(grid->ctx->device);
    GridMeshAttr m{};
    m.points = a->points;
    m.n = a->n;
    m.mask = a->mask;
    m.color_mode = a->color_mode;
    for (int k = 0; k < 3; ++k) m.view[k] = a->view[k];
    m.normals = a->normals;
    m.colors = a->colors;
    HIP_TRY(launch_grid_mesh_attributes(grid->g, grid->pal, grid->half, grid->palette, m, (hipStream_t)a->stream));
    return NERF_OK;
}

}  // extern "C"
