// C ABI of the sparse voxel grid (include/nerf_mi355x.h, "Sparse voxel grid"): argument checks and launches, and the checks
// the other grid_*_api.cpp files share (grid_internal.h). Every check that needs no device comes before the first dereference
// of a handle and before any launch.
#include <cmath>
#include <new>

#include "ctx_internal.h"
#include "grid_internal.h"

using namespace nerf;

int nerf::require_ctx(const char* fn, const nerf_ctx* c) {
    if (c) return NERF_OK;
    set_error("%s: NULL context", fn);
    return NERF_E_INVALID;
}

int nerf::require_grid(const char* fn, const nerf_sparse_grid* grid) {
    if (grid) return NERF_OK;
    set_error("%s: NULL grid", fn);
    return NERF_E_INVALID;
}

int nerf::refuse_palette_grid(const char* fn, const nerf_sparse_grid* grid) {
    if (!grid->palette) return NERF_OK;
    set_error("%s: a palette grid (nerf_grid_create_palette) is for rendering and sampling: train, differentiate and resample "
              "a grid of nerf_grid_create on the dequantised table", fn);
    return NERF_E_INVALID;
}

int nerf::refuse_half_grid(const char* fn, const nerf_sparse_grid* grid) {
    if (grid->palette) return refuse_palette_grid(fn, grid);
    if (!grid->half) return NERF_OK;
    set_error("%s: a half-precision grid (nerf_grid_create_half) has no fp32 SH table to read or write: widen it with "
              "nerf_grid_unpack_half and use a grid of nerf_grid_create", fn);
    return NERF_E_INVALID;
}

int nerf::check_grid_links(const char* fn, const int32_t* links, int64_t n, int64_t capacity, hipStream_t s) {
    int* d_bad = nullptr;
    int bad = 0;
    HIP_TRY(hipMalloc((void**)&d_bad, sizeof(int)));
    hipError_t e = launch_grid_check_links(links, n, capacity, d_bad, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d_bad);
    if (e != hipSuccess) {
        set_error("%s: %s", fn, hipGetErrorString(e));
        return NERF_E_HIP;
    }
    if (bad) {
        set_error("%s: links holds a value >= capacity = %lld", fn, (long long)capacity);
        return NERF_E_INVALID;
    }
    return NERF_OK;
}

int nerf::check_grid_reso(const char* fn, const int32_t* reso, int64_t* nodes) {
    if (!reso) {
        set_error("%s: reso is NULL", fn);
        return NERF_E_INVALID;
    }
    for (int k = 0; k < 3; ++k)
        if (reso[k] < 2 || reso[k] > 1024) {
            set_error("%s: reso[%d] = %d outside [2, 1024]", fn, k, reso[k]);
            return NERF_E_INVALID;
        }
    *nodes = (int64_t)reso[0] * reso[1] * reso[2];
    if (*nodes > kGridMaxLattice) {
        set_error("%s: %lld nodes, at most 2^30", fn, (long long)*nodes);
        return NERF_E_INVALID;
    }
    return NERF_OK;
}

int nerf::check_grid_options(const char* fn, const nerf_grid_render_options* o, GridRenderOpt* out) {
    NERF_CHECK_STRUCT(fn, o, nerf_grid_render_options);
    if (o->last_sample_opaque || o->randomize) {
        set_error("%s: %s is not built", fn, o->last_sample_opaque ? "last_sample_opaque" : "randomize");
        return NERF_E_INVALID;
    }
    if (!(o->step_size >= 1e-3f) || !std::isfinite(o->step_size) || std::isnan(o->sigma_thresh) || std::isnan(o->stop_thresh) ||
        !std::isfinite(o->background_brightness) || !std::isfinite(o->near_clip)) {
        set_error("%s: step_size = %g must be finite and >= 1e-3, the thresholds not NaN, background_brightness and near_clip finite",
                  fn, o->step_size);
        return NERF_E_INVALID;
    }
    *out = GridRenderOpt{o->step_size, o->sigma_thresh, o->stop_thresh, o->background_brightness, o->near_clip};
    return NERF_OK;
}

int nerf::check_ndc_coeffs(const char* fn, const float c[2], bool* use) {
    *use = c[0] > 0.0f;
    if (!std::isfinite(c[0]) || !std::isfinite(c[1]) || (*use && !(c[1] > 0.0f))) {
        set_error("%s: ndc_coeffs = (%g, %g) must be finite, and both positive (NDC) or the first <= 0 (no NDC)", fn, c[0], c[1]);
        return NERF_E_INVALID;
    }
    return NERF_OK;
}

int nerf::refuse_ndc_camera(const char* fn, const GridCam& cam, const char* why) {
    if (!(cam.ndc[0] > 0.0f)) return NERF_OK;
    set_error("%s: an NDC camera (ndc_coeffs > 0) is refused: %s", fn, why);
    return NERF_E_INVALID;
}

int nerf::check_grid_camera(const char* fn, const nerf_grid_camera* cam, GridCam* out) {
    NERF_CHECK_STRUCT(fn, cam, nerf_grid_camera);
    if (cam->width < 1 || cam->height < 1 || (int64_t)cam->width * cam->height > kGridMaxItems || !(std::fabs(cam->fx) > 0.0) ||
        !(std::fabs(cam->fy) > 0.0) || !std::isfinite(cam->fx) || !std::isfinite(cam->fy) || !std::isfinite(cam->cx) ||
        !std::isfinite(cam->cy)) {
        set_error("%s: camera %d x %d (at most 2^26 pixels), fx = %g, fy = %g, cx = %g, cy = %g is not usable", fn, cam->width, cam->height, cam->fx,
                  cam->fy, cam->cx, cam->cy);
        return NERF_E_INVALID;
    }
    bool ndc = false;
    const int rc = check_ndc_coeffs(fn, cam->ndc_coeffs, &ndc);
    if (rc != NERF_OK) return rc;
    out->ndc[0] = ndc ? cam->ndc_coeffs[0] : 0.0f;
    out->ndc[1] = ndc ? cam->ndc_coeffs[1] : 0.0f;
    for (int i = 0; i < 12; ++i) out->c2w[i] = (double)cam->c2w[i];
    out->fx = cam->fx;
    out->fy = cam->fy;
    out->cx = cam->cx;
    out->cy = cam->cy;
    out->width = cam->width;
    out->height = cam->height;
    return NERF_OK;
}

namespace {

int render(const char* fn, nerf_sparse_grid* grid, const nerf_grid_camera* cam, const nerf_grid_render_options* opt,
           const nerf_grid_render_args* a) {
    int rc = require_grid(fn, grid);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_render_args);
    GridRenderOpt o{};
    rc = check_grid_options(fn, opt, &o);
    if (rc != NERF_OK) return rc;
    GridRender r{};
    if (cam) {
        rc = check_grid_camera(fn, cam, &r.cam);
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
    if (r.n_rays > 0 && !a->rgb) {
        set_error("%s: rgb is NULL", fn);
        return NERF_E_INVALID;
    }
    r.rgb = a->rgb;
    r.log_transmit = a->log_transmit;
    r.counters = a->counters;
    GridDev g = grid->g;
    g.skip = a->use_skip ? grid->d_skip : nullptr;
    DeviceGuard dg(grid->ctx->device);
    if (grid->palette)
        HIP_TRY(launch_grid_palette_render(g, grid->pal, o, r, (hipStream_t)a->stream));
    else if (grid->half)
        HIP_TRY(launch_grid_half_render(g, o, r, grid->half_pair, (hipStream_t)a->stream));
    else
        HIP_TRY(launch_grid_render(g, o, r, (hipStream_t)a->stream));
    return NERF_OK;
}

}  // namespace

extern "C" {

void nerf_grid_destroy(nerf_sparse_grid* grid) {
    if (!grid) return;
    if (grid->ctx && grid->d_skip) {
        DeviceGuard g(grid->ctx->device);
        (void)hipDeviceSynchronize();
        (void)hipFree(grid->d_skip);
    }
    delete grid;
}

int nerf_grid_create(nerf_ctx* c, const nerf_sparse_grid_desc* d, nerf_sparse_grid** out) {
    const char* fn = "nerf_grid_create";
    if (!c || !out) {
        set_error("nerf_grid_create: NULL argument");
        return NERF_E_INVALID;
    }
    *out = nullptr;
    NERF_CHECK_STRUCT(fn, d, nerf_sparse_grid_desc);
    if (d->basis_dim != 1 && d->basis_dim != 4 && d->basis_dim != 9) {
        set_error("nerf_grid_create: basis_dim = %d: spherical harmonics of 1, 4 or 9 coefficients are built", d->basis_dim);
        return NERF_E_INVALID;
    }
    int64_t n = 0;
    float offset[3], scaling[3];
    int rc = check_grid_reso(fn, d->reso, &n);
    if (rc == NERF_OK) rc = grid_world2grid(fn, d->center, d->radius, d->reso, offset, scaling);
    if (rc != NERF_OK) return rc;
    if (d->capacity < 0 || d->capacity > 0x7fffffffLL || !d->links || (d->capacity > 0 && (!d->density_data || !d->sh_data))) {
        set_error("nerf_grid_create: links, and with capacity = %lld > 0 density_data and sh_data, are required",
                  (long long)d->capacity);
        return NERF_E_INVALID;
    }
    DeviceGuard dg(c->device);
    rc = check_grid_links(fn, d->links, n, d->capacity, (hipStream_t)d->stream);
    if (rc != NERF_OK) return rc;
    nerf_sparse_grid* grid = new (std::nothrow) nerf_sparse_grid();
    if (!grid) return NERF_E_NOMEM;
    grid->ctx = c;
    GridDev& g = grid->g;
    g.links = d->links;
    g.density = d->density_data;
    g.sh = d->sh_data;
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

int nerf_grid_render_rays(nerf_sparse_grid* grid, const nerf_grid_render_options* opt, const nerf_grid_render_args* args) {
    return render("nerf_grid_render_rays", grid, nullptr, opt, args);
}

int nerf_grid_render_image(nerf_sparse_grid* grid, const nerf_grid_camera* cam, const nerf_grid_render_options* opt,
                           const nerf_grid_render_args* args) {
    if (!cam) {
        set_error("nerf_grid_render_image: nerf_grid_camera is NULL");
        return NERF_E_INVALID;
    }
    return render("nerf_grid_render_image", grid, cam, opt, args);
}

int nerf_grid_gen_rays(nerf_ctx* c, const nerf_grid_camera* cam, float* origins, float* dirs, void* stream) {
    if (!c || !origins || !dirs) {
        set_error("nerf_grid_gen_rays: NULL argument");
        return NERF_E_INVALID;
    }
    GridCam gc{};
    const int rc = check_grid_camera("nerf_grid_gen_rays", cam, &gc);
    if (rc != NERF_OK) return rc;
    DeviceGuard dg(c->device);
    HIP_TRY(launch_grid_gen_rays(gc, origins, dirs, (hipStream_t)stream));
    return NERF_OK;
}

int nerf_grid_rays_to_ndc(nerf_ctx* c, const nerf_grid_rays_to_ndc_args* a) {
    const char* fn = "nerf_grid_rays_to_ndc";
    int rc = require_ctx(fn, c);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_rays_to_ndc_args);
    if (a->n < 0 || a->n > kGridMaxItems || (a->n > 0 && (!a->origins || !a->dirs || !a->origins_out || !a->dirs_out))) {
        set_error("%s: n = %lld must be in [0, 2^26] and needs origins, dirs, origins_out and dirs_out", fn, (long long)a->n);
        return NERF_E_INVALID;
    }
    bool ndc = false;
    rc = check_ndc_coeffs(fn, a->ndc_coeffs, &ndc);
    if (rc != NERF_OK) return rc;
    if (!ndc) {
        set_error("%s: ndc_coeffs = (%g, %g) must both be positive", fn, a->ndc_coeffs[0], a->ndc_coeffs[1]);
        return NERF_E_INVALID;
    }
    if (a->n == 0) return NERF_OK;
    // ---- from here on the context is read ----
    DeviceGuard dg(c->device);
    HIP_TRY(launch_grid_rays_to_ndc(a->origins, a->dirs, a->n, a->ndc_coeffs[0], a->ndc_coeffs[1], a->origins_out, a->dirs_out,
                                    (hipStream_t)a->stream));
    return NERF_OK;
}

int nerf_grid_sample(nerf_sparse_grid* grid, const nerf_grid_sample_args* a) {
    const int rc = require_grid("nerf_grid_sample", grid);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT("nerf_grid_sample", a, nerf_grid_sample_args);
    if (a->n < 0 || a->n > kGridMaxItems || (a->n > 0 && (!a->points || !a->density || (a->want_colors && !a->sh)))) {
        set_error("nerf_grid_sample: n = %lld must be in [0, 2^26] and needs points, density and (with want_colors) sh", (long long)a->n);
        return NERF_E_INVALID;
    }
    DeviceGuard dg(grid->ctx->device);
    if (grid->palette)
        HIP_TRY(launch_grid_palette_sample(grid->g, grid->pal, a->points, a->n, a->grid_coords, a->want_colors, a->density, a->sh,
                                           (hipStream_t)a->stream));
    else if (grid->half)
        HIP_TRY(launch_grid_half_sample(grid->g, a->points, a->n, a->grid_coords, a->want_colors, a->density, a->sh,
                                        (hipStream_t)a->stream));
    else
        HIP_TRY(launch_grid_sample(grid->g, a->points, a->n, a->grid_coords, a->want_colors, a->density, a->sh, (hipStream_t)a->stream));
    return NERF_OK;
}

int nerf_grid_accelerate(nerf_sparse_grid* grid, void* stream) {
    const int rc = require_grid("nerf_grid_accelerate", grid);
    if (rc != NERF_OK) return rc;
    DeviceGuard dg(grid->ctx->device);
    const size_t n = (size_t)grid->g.size[0] * grid->g.size[1] * grid->g.size[2];
    if (!grid->d_skip) {
        hipError_t e = hipMalloc((void**)&grid->d_skip, n);
        if (e != hipSuccess) {
            grid->d_skip = nullptr;
            set_error("nerf_grid_accelerate: hipMalloc(%zu) failed: %s", n, hipGetErrorString(e));
            return NERF_E_NOMEM;
        }
    }
    HIP_TRY(launch_grid_accelerate(grid->g, grid->d_skip, (hipStream_t)stream));
    return NERF_OK;
}

int nerf_grid_drop_skip(nerf_sparse_grid* grid) {
    const int rc = require_grid("nerf_grid_drop_skip", grid);
    if (rc != NERF_OK) return rc;
    if (!grid->d_skip) return NERF_OK;
    DeviceGuard dg(grid->ctx->device);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipFree(grid->d_skip));
    grid->d_skip = nullptr;
    return NERF_OK;
}

int nerf_grid_has_skip(const nerf_sparse_grid* grid) { return grid && grid->d_skip ? 1 : 0; }

int nerf_grid_project_sh(nerf_ctx* c, const nerf_grid_project_args* a) {
    const int rc = require_ctx("nerf_grid_project_sh", c);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT("nerf_grid_project_sh", a, nerf_grid_project_args);
    if ((a->basis_dim != 1 && a->basis_dim != 4 && a->basis_dim != 9) || a->n_dirs < 1 || a->basis_dim * a->n_dirs > 4096 ||
        a->m < 0 || a->m > kGridMaxItems || a->row0 < 0 || (a->m > 0 && (!a->raw || !a->P || !a->sh_out))) {
        set_error("nerf_grid_project_sh: basis_dim = %d in {1, 4, 9}, 1 <= n_dirs = %d, basis_dim * n_dirs <= 4096, m = %lld "
                  "and non-NULL raw, P, sh_out are required", a->basis_dim, a->n_dirs, (long long)a->m);
        return NERF_E_INVALID;
    }
    DeviceGuard dg(c->device);
    HIP_TRY(launch_grid_project_sh(a->raw, a->m, a->n_dirs, a->basis_dim, a->P, a->sh_out, a->row0, (hipStream_t)a->stream));
    return NERF_OK;
}

}  // extern "C"
