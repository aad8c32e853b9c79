// C ABI of the PlenOctree (include/nerf_mi355x.h, "PlenOctree"): argument checks and launches. Every check that needs no
// launch comes before the first launch; the pointer checks ask the runtime where an array lives and launch nothing.
#include <cmath>
#include <new>

#include "ctx_internal.h"
#include "octree_internal.h"

using namespace nerf;

namespace {

// NERF_OK where `p` is device memory of GPU `device`
int require_device_array(const char* fn, const char* name, const void* p, int device) {
    if (!p) {
        set_error("%s: %s is NULL", fn, name);
        return NERF_E_INVALID;
    }
    hipPointerAttribute_t attr{};
    const hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) (void)hipGetLastError();      // (an address the runtime does not know: host memory)
    if (e != hipSuccess || attr.type != hipMemoryTypeDevice || attr.device != device) {
        set_error("%s: %s is not device memory of GPU %d", fn, name, device);
        return NERF_E_INVALID;
    }
    return NERF_OK;
}

int basis_of(int data_dim) {
    for (int b : {1, 4, 9, 16, 25})
        if (data_dim == 3 * b + 1) return b;
    return 0;
}

int check_options(const char* fn, const nerf_octree_render_options* o, OctreeRenderOpt* out) {
    NERF_CHECK_STRUCT(fn, o, nerf_octree_render_options);
    if (!(o->step_size > 0.0f) || !std::isfinite(o->step_size) || std::isnan(o->sigma_thresh) || std::isnan(o->stop_thresh) ||
        !std::isfinite(o->background_brightness)) {
        set_error("%s: step_size = %g must be positive and finite, the thresholds not NaN, background_brightness finite", fn,
                  o->step_size);
        return NERF_E_INVALID;
    }
    *out = OctreeRenderOpt{o->step_size, o->sigma_thresh, o->stop_thresh, o->background_brightness};
    return NERF_OK;
}

int render(const char* fn, nerf_octree* tree, const nerf_grid_camera* cam, const nerf_octree_render_options* opt,
           const nerf_octree_render_args* a) {
    if (!tree) {
        set_error("%s: NULL tree", fn);
        return NERF_E_INVALID;
    }
    NERF_CHECK_STRUCT(fn, a, nerf_octree_render_args);
    OctreeRenderOpt o{};
    int rc = check_options(fn, opt, &o);
    if (rc != NERF_OK) return rc;
    OctreeRender r{};
    if (cam) {
        rc = check_grid_camera(fn, cam, &r.cam);
        if (rc == NERF_OK) rc = refuse_ndc_camera(fn, r.cam, "NDC is not built for the octree");
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
    if (r.n_rays == 0) return NERF_OK;
    DeviceGuard dg(tree->ctx->device);
    const int dev = tree->ctx->device;
    if (!cam) {
        rc = require_device_array(fn, "origins", a->origins, dev);
        if (rc == NERF_OK) rc = require_device_array(fn, "dirs", a->dirs, dev);
        if (rc != NERF_OK) return rc;
    }
    rc = require_device_array(fn, "rgb", a->rgb, dev);
    if (rc == NERF_OK && a->steps) rc = require_device_array(fn, "steps", a->steps, dev);
    if (rc == NERF_OK && a->capped) rc = require_device_array(fn, "capped", a->capped, dev);
    if (rc != NERF_OK) return rc;
    r.rgb = a->rgb;
    r.steps = a->steps;
    r.capped = a->capped;
    HIP_TRY(launch_octree_render(tree->t, o, r, (hipStream_t)a->stream));
    return NERF_OK;
}

int backward(const char* fn, nerf_octree* tree, const nerf_grid_camera* cam, const nerf_octree_render_options* opt,
             const nerf_octree_backward_args* a) {
    if (!tree) {
        set_error("%s: NULL tree", fn);
        return NERF_E_INVALID;
    }
    NERF_CHECK_STRUCT(fn, a, nerf_octree_backward_args);
    OctreeRenderOpt o{};
    int rc = check_options(fn, opt, &o);
    if (rc != NERF_OK) return rc;
    OctreeBackward b{};
    if (cam) {
        rc = check_grid_camera(fn, cam, &b.cam);
        if (rc == NERF_OK) rc = refuse_ndc_camera(fn, b.cam, "NDC is not built for the octree");
        if (rc != NERF_OK) return rc;
        b.n_rays = (int64_t)cam->width * cam->height;
    } else {
        if (a->n_rays < 0 || a->n_rays > kGridMaxItems || (a->n_rays > 0 && (!a->origins || !a->dirs))) {
            set_error("%s: n_rays = %lld must be in [0, 2^26] and needs origins and dirs", fn, (long long)a->n_rays);
            return NERF_E_INVALID;
        }
        b.origins = a->origins;
        b.dirs = a->dirs;
        b.n_rays = a->n_rays;
    }
    if ((a->grad_rgb != nullptr) == (a->rgb_gt != nullptr)) {
        set_error("%s: exactly one of grad_rgb and rgb_gt is required", fn);
        return NERF_E_INVALID;
    }
    if (!a->grad_data) {
        set_error("%s: grad_data is NULL", fn);
        return NERF_E_INVALID;
    }
    if (!std::isfinite(a->loss_scale)) {
        set_error("%s: loss_scale = %g must be finite", fn, a->loss_scale);
        return NERF_E_INVALID;
    }
    if (b.n_rays == 0) return NERF_OK;
    DeviceGuard dg(tree->ctx->device);
    const int dev = tree->ctx->device;
    if (!cam) {
        rc = require_device_array(fn, "origins", a->origins, dev);
        if (rc == NERF_OK) rc = require_device_array(fn, "dirs", a->dirs, dev);
        if (rc != NERF_OK) return rc;
    }
    rc = a->grad_rgb ? require_device_array(fn, "grad_rgb", a->grad_rgb, dev) : require_device_array(fn, "rgb_gt", a->rgb_gt, dev);
    if (rc == NERF_OK) rc = require_device_array(fn, "grad_data", a->grad_data, dev);
    if (rc == NERF_OK && a->loss) rc = require_device_array(fn, "loss", a->loss, dev);
    if (rc == NERF_OK && a->rgb) rc = require_device_array(fn, "rgb", a->rgb, dev);
    if (rc == NERF_OK && a->capped) rc = require_device_array(fn, "capped", a->capped, dev);
    if (rc != NERF_OK) return rc;
    b.grad_rgb = a->grad_rgb;
    b.rgb_gt = a->rgb_gt;
    b.loss_scale = a->loss_scale;
    b.grad_data = a->grad_data;
    b.loss = a->loss;
    b.rgb = a->rgb;
    b.capped = a->capped;
    HIP_TRY(launch_octree_backward(tree->t, o, b, (hipStream_t)a->stream));
    return NERF_OK;
}

int levels_of(int reso) {
    for (int l = 1; l <= 10; ++l)
        if (reso == 1 << l) return l;
    return 0;
}

}  // namespace

extern "C" {

void nerf_octree_destroy(nerf_octree* tree) {
    if (!tree) return;
    if (tree->ctx && tree->d_table) {
        DeviceGuard g(tree->ctx->device);
        (void)hipDeviceSynchronize();
        (void)hipFree(tree->d_table);
    }
    delete tree;
}

int nerf_octree_accelerate(nerf_octree* tree, int32_t levels, void* stream) {
    const char* fn = "nerf_octree_accelerate";
    if (!tree) {
        set_error("%s: NULL tree", fn);
        return NERF_E_INVALID;
    }
    if (levels < 0 || levels > 8) {
        set_error("%s: levels = %d must be in [0, 8] (0 drops the table)", fn, levels);
        return NERF_E_INVALID;
    }
    DeviceGuard dg(tree->ctx->device);
    if (tree->d_table) {      // a table of another size, or none: renders in flight may still read the old one
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipFree(tree->d_table));
        tree->d_table = nullptr;
        tree->t.table = nullptr;
        tree->t.table_levels = 0;
    }
    const int k = levels < tree->t.max_depth ? levels : tree->t.max_depth;
    if (k < 1) return NERF_OK;      // a root-only tree has nothing to skip
    const size_t bytes = ((size_t)1 << (3 * k)) * sizeof(int2);
    hipError_t e = hipMalloc((void**)&tree->d_table, bytes);
    if (e != hipSuccess) {
        tree->d_table = nullptr;
        set_error("%s: hipMalloc(%zu) failed: %s", fn, bytes, hipGetErrorString(e));
        return NERF_E_NOMEM;
    }
    HIP_TRY(launch_octree_table(tree->t, k, tree->d_table, (hipStream_t)stream));
    tree->t.table = tree->d_table;
    tree->t.table_levels = k;
    return NERF_OK;
}

int nerf_octree_table_levels(const nerf_octree* tree) { return tree ? tree->t.table_levels : 0; }

int nerf_octree_create(nerf_ctx* c, const nerf_octree_desc* d, nerf_octree** out) {
    const char* fn = "nerf_octree_create";
    if (!c || !out) {
        set_error("%s: NULL argument", fn);
        return NERF_E_INVALID;
    }
    *out = nullptr;
    NERF_CHECK_STRUCT(fn, d, nerf_octree_desc);
    const int B = basis_of(d->data_dim);
    if (!B) {
        set_error("%s: data_dim = %d: spherical harmonics of 1, 4, 9, 16 or 25 coefficients are built (data_dim = 3 B + 1)", fn,
                  d->data_dim);
        return NERF_E_INVALID;
    }
    if (d->n_nodes < 1 || d->n_nodes > kOctreeMaxNodes || d->max_depth < 0 || d->max_depth > NERF_OCTREE_MAX_DEPTH) {
        set_error("%s: n_nodes = %lld must be in [1, 2^27], max_depth = %d in [0, %d]", fn, (long long)d->n_nodes, d->max_depth,
                  NERF_OCTREE_MAX_DEPTH);
        return NERF_E_INVALID;
    }
    if (d->rgb_activation != NERF_OCTREE_RGB_SIGMOID && d->rgb_activation != NERF_OCTREE_RGB_RELU_HALF) {
        set_error("%s: rgb_activation = %d is neither NERF_OCTREE_RGB_SIGMOID nor NERF_OCTREE_RGB_RELU_HALF", fn, d->rgb_activation);
        return NERF_E_INVALID;
    }
    for (int k = 0; k < 3; ++k)
        if (!(d->invradius[k] > 0.0f) || !std::isfinite(d->invradius[k]) || !std::isfinite(d->offset[k])) {
            set_error("%s: axis %d: invradius = %g must be positive and finite, offset = %g finite", fn, k, d->invradius[k],
                      d->offset[k]);
            return NERF_E_INVALID;
        }
    DeviceGuard dg(c->device);
    int rc = require_device_array(fn, "child", d->child, c->device);
    if (rc == NERF_OK) rc = require_device_array(fn, "data", d->data, c->device);
    if (rc != NERF_OK) return rc;
    hipStream_t s = (hipStream_t)d->stream;
    int bad = 0;
    hipError_t e = hipSuccess;
    {      // the flag lives in the context's workspace: no allocation, and no hipFree (a device-wide wait) per create
        ScratchScope scope(c, s);
        HIP_TRY(scope.status);
        rc = ensure_workspace(c, 256);
        if (rc != NERF_OK) return rc;
        int* d_bad = (int*)c->ws;
        e = launch_octree_check_child(d->child, d->n_nodes, d_bad, s);
        if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
    if (e != hipSuccess) {
        set_error("%s: %s", fn, hipGetErrorString(e));
        return NERF_E_HIP;
    }
    if (bad) {
        set_error("%s: child holds a negative entry or one that points past n_nodes = %lld", fn, (long long)d->n_nodes);
        return NERF_E_INVALID;
    }
    nerf_octree* tree = new (std::nothrow) nerf_octree();
    if (!tree) return NERF_E_NOMEM;
    tree->ctx = c;
    OctreeDev& t = tree->t;
    t.child = d->child;
    t.data = d->data;
    t.n_nodes = d->n_nodes;
    t.data_dim = d->data_dim;
    t.basis_dim = B;
    t.max_depth = d->max_depth;
    t.act = d->rgb_activation;
    t.table = nullptr;
    t.table_levels = 0;
    for (int k = 0; k < 3; ++k) {
        t.invradius[k] = d->invradius[k];
        t.offset[k] = d->offset[k];
    }
    *out = tree;
    return NERF_OK;
}

int nerf_octree_render_rays(nerf_octree* tree, const nerf_octree_render_options* opt, const nerf_octree_render_args* args) {
    return render("nerf_octree_render_rays", tree, nullptr, opt, args);
}

int nerf_octree_render_image(nerf_octree* tree, const nerf_grid_camera* cam, const nerf_octree_render_options* opt,
                             const nerf_octree_render_args* args) {
    if (!cam) {
        set_error("nerf_octree_render_image: nerf_grid_camera is NULL");
        return NERF_E_INVALID;
    }
    return render("nerf_octree_render_image", tree, cam, opt, args);
}

int nerf_octree_backward_rays(nerf_octree* tree, const nerf_octree_render_options* opt, const nerf_octree_backward_args* args) {
    return backward("nerf_octree_backward_rays", tree, nullptr, opt, args);
}

int nerf_octree_backward_image(nerf_octree* tree, const nerf_grid_camera* cam, const nerf_octree_render_options* opt,
                               const nerf_octree_backward_args* args) {
    if (!cam) {
        set_error("nerf_octree_backward_image: nerf_grid_camera is NULL");
        return NERF_E_INVALID;
    }
    return backward("nerf_octree_backward_image", tree, cam, opt, args);
}

int64_t nerf_octree_build_workspace(int32_t reso) {
    const int L = levels_of(reso);
    if (!L) return -1;
    OctreeBuildLayout lay{};
    octree_build_layout(L, &lay);
    return (int64_t)lay.total;
}

int nerf_octree_build_from_grid(nerf_sparse_grid* grid, const nerf_octree_build_args* a) {
    const char* fn = "nerf_octree_build_from_grid";
    int rc = require_grid(fn, grid);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_octree_build_args);
    rc = refuse_half_grid(fn, grid);
    if (rc != NERF_OK) return rc;
    const GridDev& g = grid->g;
    const int L = g.size[0] == g.size[1] && g.size[1] == g.size[2] ? levels_of(g.size[0]) : 0;
    if (!L) {
        set_error("%s: the grid is %d x %d x %d: an octree needs a cube whose side is a power of two", fn, g.size[0], g.size[1],
                  g.size[2]);
        return NERF_E_INVALID;
    }
    OctreeBuild b{};
    octree_build_layout(L, &b.lay);
    if (!a->workspace || a->workspace_bytes < (int64_t)b.lay.total || !a->n_nodes) {
        set_error("%s: workspace of %zu bytes (nerf_octree_build_workspace) and n_nodes are required", fn, b.lay.total);
        return NERF_E_INVALID;
    }
    const bool fill = a->child != nullptr;
    if (fill && (!a->parent_depth || !a->data || *a->n_nodes < 1 || *a->n_nodes > kOctreeMaxNodes)) {
        set_error("%s: the filling call needs child, parent_depth and data of n_nodes = %lld nodes in [1, 2^27]", fn,
                  (long long)*a->n_nodes);
        return NERF_E_INVALID;
    }
    DeviceGuard dg(grid->ctx->device);
    const int dev = grid->ctx->device;
    rc = require_device_array(fn, "workspace", a->workspace, dev);
    if (rc == NERF_OK && fill) rc = require_device_array(fn, "child", a->child, dev);
    if (rc == NERF_OK && fill) rc = require_device_array(fn, "parent_depth", a->parent_depth, dev);
    if (rc == NERF_OK && fill) rc = require_device_array(fn, "data", a->data, dev);
    if (rc != NERF_OK) return rc;
    b.links = g.links;
    b.density = g.density;
    b.sh = g.sh;
    b.basis_dim = g.basis_dim;
    b.levels = L;
    b.ws = (char*)a->workspace;
    hipStream_t s = (hipStream_t)a->stream;
    if (!fill) {
        HIP_TRY(launch_octree_plan(b, s));
        int32_t n = 0;
        HIP_TRY(hipMemcpyAsync(&n, b.ws + b.lay.base + L * sizeof(int32_t), sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        *a->n_nodes = n;
        return NERF_OK;
    }
    b.child = a->child;
    b.parent_depth = a->parent_depth;
    b.data = a->data;
    b.n_nodes = *a->n_nodes;
    HIP_TRY(launch_octree_fill(b, s));
    return NERF_OK;
}

}  // extern "C"
