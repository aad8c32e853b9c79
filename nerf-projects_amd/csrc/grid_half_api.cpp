// C ABI of the half-precision colour table (include/nerf_mi355x.h, "Sparse voxel grid: half-precision colours"): pack, unpack
// and nerf_grid_create_half. Rendering and sampling such a grid are nerf_grid_render_* / nerf_grid_sample of grid_api.cpp,
// which look at the handle. Every check that needs no device comes before the first launch.
#include <new>

#include "ctx_internal.h"
#include "grid_internal.h"

using namespace nerf;

namespace {

// The render kernel's lane mapping behind NERF_GRID_HALF_LANES_DEFAULT: the faster one in profiles/grid_half_ab.md.
constexpr bool kDefaultPair = true;

int check_basis(const char* fn, int basis_dim) {
    if (basis_dim == 1 || basis_dim == 4 || basis_dim == 9) return NERF_OK;
    set_error("%s: basis_dim = %d: spherical harmonics of 1, 4 or 9 coefficients are built", fn, basis_dim);
    return NERF_E_INVALID;
}

}  // namespace

extern "C" {

int nerf_grid_half_row_halfs(int32_t basis_dim) {
    const int rc = check_basis("nerf_grid_half_row_halfs", basis_dim);
    return rc != NERF_OK ? rc : grid_half_row_halfs(basis_dim);
}

int nerf_grid_pack_half(nerf_ctx* c, const nerf_grid_pack_half_args* a) {
    const char* fn = "nerf_grid_pack_half";
    int rc = require_ctx(fn, c);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_pack_half_args);
    rc = check_basis(fn, a->basis_dim);
    if (rc != NERF_OK) return rc;
    if (a->capacity < 0 || a->capacity > 0x7fffffffLL) {
        set_error("%s: capacity = %lld must be in [0, 2^31)", fn, (long long)a->capacity);
        return NERF_E_INVALID;
    }
    if (a->rows < 0) {
        set_error("%s: rows = %lld must not be negative", fn, (long long)a->rows);
        return NERF_E_INVALID;
    }
    if (a->row0 < 0 || a->row0 > a->capacity || a->rows > a->capacity - a->row0) {
        set_error("%s: row0 = %lld, rows = %lld: row0 + rows must lie in [0, capacity = %lld]", fn, (long long)a->row0,
                  (long long)a->rows, (long long)a->capacity);
        return NERF_E_INVALID;
    }
    if (a->rows > 0 && !a->sh_data) {
        set_error("%s: sh_data is NULL", fn);
        return NERF_E_INVALID;
    }
    if (a->rows > 0 && (!a->sh_half || ((uintptr_t)a->sh_half & 3))) {
        set_error("%s: sh_half is NULL or not 4-byte aligned", fn);
        return NERF_E_INVALID;
    }
    if (a->rows == 0) return NERF_OK;
    GridHalfPack p{a->sh_data, a->sh_half, a->rows, a->row0, a->basis_dim, a->clamped};
    DeviceGuard dg(c->device);
    HIP_TRY(launch_grid_pack_half(p, (hipStream_t)a->stream));
    return NERF_OK;
}

int nerf_grid_unpack_half(nerf_ctx* c, const uint16_t* sh_half, int64_t rows, int32_t basis_dim, float* sh_data, void* stream) {
    const char* fn = "nerf_grid_unpack_half";
    int rc = require_ctx(fn, c);
    if (rc == NERF_OK) rc = check_basis(fn, basis_dim);
    if (rc != NERF_OK) return rc;
    if (rows < 0 || rows > 0x7fffffffLL) {
        set_error("%s: rows = %lld must be in [0, 2^31)", fn, (long long)rows);
        return NERF_E_INVALID;
    }
    if (rows > 0 && !sh_half) {
        set_error("%s: sh_half is NULL", fn);
        return NERF_E_INVALID;
    }
    if (rows > 0 && !sh_data) {
        set_error("%s: sh_data is NULL", fn);
        return NERF_E_INVALID;
    }
    if (rows == 0) return NERF_OK;
    DeviceGuard dg(c->device);
    HIP_TRY(launch_grid_unpack_half(sh_half, rows, basis_dim, sh_data, (hipStream_t)stream));
    return NERF_OK;
}

int nerf_grid_create_half(nerf_ctx* c, const nerf_grid_half_desc* d, nerf_sparse_grid** out) {
    const char* fn = "nerf_grid_create_half";
    if (!c || !out) {
        set_error("%s: NULL argument", fn);
        return NERF_E_INVALID;
    }
    *out = nullptr;
    NERF_CHECK_STRUCT(fn, d, nerf_grid_half_desc);
    int rc = check_basis(fn, d->basis_dim);
    if (rc != NERF_OK) return rc;
    if (d->lanes != NERF_GRID_HALF_LANES_DEFAULT && d->lanes != NERF_GRID_HALF_LANES_SINGLE && d->lanes != NERF_GRID_HALF_LANES_PAIR) {
        set_error("%s: lanes = %d must be one of NERF_GRID_HALF_LANES_*", fn, d->lanes);
        return NERF_E_INVALID;
    }
    int64_t n = 0;
    float offset[3], scaling[3];
    rc = check_grid_reso(fn, d->reso, &n);
    if (rc == NERF_OK) rc = grid_world2grid(fn, d->center, d->radius, d->reso, offset, scaling);
    if (rc != NERF_OK) return rc;
    if (d->capacity < 0 || d->capacity > 0x7fffffffLL || !d->links || (d->capacity > 0 && (!d->density_data || !d->sh_half))) {
        set_error("%s: links, and with capacity = %lld > 0 density_data and sh_half, are required", fn, (long long)d->capacity);
        return NERF_E_INVALID;
    }
    if ((uintptr_t)d->sh_half & 3) {
        set_error("%s: sh_half is not 4-byte aligned", fn);
        return NERF_E_INVALID;
    }
    DeviceGuard dg(c->device);
    rc = check_grid_links(fn, d->links, n, d->capacity, (hipStream_t)d->stream);
    if (rc != NERF_OK) return rc;
    nerf_sparse_grid* grid = new (std::nothrow) nerf_sparse_grid();
    if (!grid) return NERF_E_NOMEM;
    grid->ctx = c;
    grid->half = true;
    grid->half_pair = d->lanes == NERF_GRID_HALF_LANES_DEFAULT ? kDefaultPair : d->lanes == NERF_GRID_HALF_LANES_PAIR;
    GridDev& g = grid->g;
    g.links = d->links;
    g.density = d->density_data;
    g.sh = nullptr;
    g.sh_half = d->sh_half;
    g.skip = nullptr;
    g.basis_dim = d->basis_dim;
    g.capacity = d->capacity;
    for (int k = 0; k < 3; ++k) {
        g.size[k] = d->reso[k];
        g.offset[k] = offset[k];
        g.scaling[k] = scaling[k];
    }
    *out = grid;
    return NERF_OK;
}

}  // extern "C"
