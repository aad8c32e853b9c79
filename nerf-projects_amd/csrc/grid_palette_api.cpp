// C ABI of the palette-quantised colours (include/nerf_mi355x.h, "Sparse voxel grid: palette-quantised colours"): the median
// cut, its workspace query and nerf_grid_create_palette. Rendering and sampling such a grid are nerf_grid_render_* /
// nerf_grid_sample of grid_api.cpp, which look at the handle. Every check that needs no device comes before the first launch.
#include <new>

#include "ctx_internal.h"
#include "grid_internal.h"

using namespace nerf;

namespace {

int check_cut_shape(const char* fn, int64_t m, int32_t bits) {
    if (m < 0 || m > 0x7fffffffLL) {
        set_error("%s: m = %lld must be in [0, 2^31)", fn, (long long)m);
        return NERF_E_INVALID;
    }
    if (bits < 1 || bits > 16) {
        set_error("%s: bits = %d must be in [1, 16]", fn, bits);
        return NERF_E_INVALID;
    }
    return NERF_OK;
}

}  // namespace

extern "C" {

int64_t nerf_grid_median_cut_workspace(int64_t m, int32_t bits) {
    const int rc = check_cut_shape("nerf_grid_median_cut_workspace", m, bits);
    if (rc != NERF_OK) return rc;
    GridMedianCutLayout l{};
    grid_median_cut_layout(m, bits, &l);
    return (int64_t)l.total;
}

int nerf_grid_quantize_median_cut(nerf_ctx* c, const nerf_grid_median_cut_args* a) {
    const char* fn = "nerf_grid_quantize_median_cut";
    int rc = require_ctx(fn, c);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_median_cut_args);
    rc = check_cut_shape(fn, a->m, a->bits);
    if (rc != NERF_OK) return rc;
    if (a->m > 0 && (!a->colors || !a->ids)) {
        set_error("%s: colors and ids are required with m = %lld > 0", fn, (long long)a->m);
        return NERF_E_INVALID;
    }
    if (!a->palette || !a->nonfinite) {
        set_error("%s: palette and nonfinite are required", fn);
        return NERF_E_INVALID;
    }
    GridMedianCutLayout l{};
    grid_median_cut_layout(a->m, a->bits, &l);
    if (!a->workspace || ((uintptr_t)a->workspace & 255) || a->workspace_bytes < (int64_t)l.total) {
        set_error("%s: workspace must be 256-byte aligned and hold nerf_grid_median_cut_workspace(m, bits) = %lld bytes, got %lld",
                  fn, (long long)l.total, (long long)a->workspace_bytes);
        return NERF_E_INVALID;
    }
    *a->nonfinite = 0;
    const GridMedianCut k{a->colors, a->m, a->bits, a->ids, a->palette, a->workspace};
    hipStream_t s = (hipStream_t)a->stream;
    DeviceGuard dg(c->device);
    HIP_TRY(launch_grid_median_cut_count(k, l, s));
    unsigned long long bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, (char*)a->workspace + l.nonfinite, sizeof(bad), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *a->nonfinite = (int64_t)bad;
    if (bad) {
        set_error("%s: %llu of the %lld colours have a NaN or an infinity: nothing was quantised", fn, bad, (long long)a->m);
        return NERF_E_INVALID;
    }
    const hipError_t e = launch_grid_median_cut(k, l, s);
    if (e == hipErrorOutOfMemory) {
        set_error("%s: the radix sort asks for more than the %zu bytes the workspace sets aside for it", fn, l.sort_bytes);
        return NERF_E_INTERNAL;
    }
    HIP_TRY(e);
    return NERF_OK;
}

int nerf_grid_create_palette(nerf_ctx* c, const nerf_grid_palette_desc* d, nerf_sparse_grid** out) {
    const char* fn = "nerf_grid_create_palette";
    if (!c || !out) {
        set_error("%s: NULL argument", fn);
        return NERF_E_INVALID;
    }
    *out = nullptr;
    NERF_CHECK_STRUCT(fn, d, nerf_grid_palette_desc);
    if (d->basis_dim != 1 && d->basis_dim != 4 && d->basis_dim != 9) {
        set_error("%s: basis_dim = %d: spherical harmonics of 1, 4 or 9 coefficients are built", fn, d->basis_dim);
        return NERF_E_INVALID;
    }
    if (d->bits < 1 || d->bits > 16 || d->retain < 0 || d->retain > d->basis_dim) {
        set_error("%s: bits = %d must be in [1, 16], retain = %d in [0, basis_dim = %d]", fn, d->bits, d->retain, d->basis_dim);
        return NERF_E_INVALID;
    }
    int64_t n = 0;
    float offset[3], scaling[3];
    int rc = check_grid_reso(fn, d->reso, &n);
    if (rc == NERF_OK) rc = grid_world2grid(fn, d->center, d->radius, d->reso, offset, scaling);
    if (rc != NERF_OK) return rc;
    const int q = d->basis_dim - d->retain;
    if (d->capacity < 0 || d->capacity > 0x7fffffffLL || !d->links || (d->capacity > 0 && !d->density_data) ||
        (d->capacity > 0 && q > 0 && !d->quant_map) || (q > 0 && !d->quant_colors) ||
        (d->capacity > 0 && d->retain > 0 && !d->data_retained)) {
        set_error("%s: links, and with capacity = %lld > 0 density_data, quant_map (and quant_colors) for the %d quantised and "
                  "data_retained for the %d retained functions, are required", fn, (long long)d->capacity, q, d->retain);
        return NERF_E_INVALID;
    }
    if (((uintptr_t)d->quant_map | (uintptr_t)d->quant_colors | (uintptr_t)d->data_retained) & 1) {
        set_error("%s: quant_map, quant_colors and data_retained must be 2-byte aligned", fn);
        return NERF_E_INVALID;
    }
    hipStream_t s = (hipStream_t)d->stream;
    DeviceGuard dg(c->device);
    rc = check_grid_links(fn, d->links, n, d->capacity, s);
    if (rc != NERF_OK) return rc;
    if (d->bits < 16 && q > 0 && d->capacity > 0) {      // (a uint16 is always < 2^16)
        int* d_bad = nullptr;
        int bad = 0;
        HIP_TRY(hipMalloc((void**)&d_bad, sizeof(int)));
        hipError_t e = launch_grid_palette_check(d->quant_map, d->capacity * q, 1 << d->bits, d_bad, s);
        if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        (void)hipFree(d_bad);
        HIP_TRY(e);
        if (bad) {
            set_error("%s: quant_map holds an index >= 2^bits = %d", fn, 1 << d->bits);
            return NERF_E_INVALID;
        }
    }
    nerf_sparse_grid* grid = new (std::nothrow) nerf_sparse_grid();
    if (!grid) return NERF_E_NOMEM;
    grid->ctx = c;
    grid->palette = true;
    grid->pal = GridPalette{d->quant_map, d->quant_colors, d->data_retained, d->retain, 1 << d->bits};
    GridDev& g = grid->g;
    g.links = d->links;
    g.density = d->density_data;
    g.sh = nullptr;
    g.sh_half = nullptr;
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
