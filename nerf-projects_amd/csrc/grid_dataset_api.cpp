// C ABI of the sparse voxel grid's training data (include/nerf_mi355x.h, "Sparse voxel grid: training data"): argument
// checks and the launch. Every check comes before the first dereference of the context and before any launch.
#include <cmath>

#include "ctx_internal.h"
#include "grid_dataset_internal.h"

using namespace nerf;

namespace {

constexpr int32_t kDatasetMaxImages = 1 << 20;
constexpr int32_t kDatasetMaxSide = 1 << 15;
constexpr int64_t kDatasetMaxRow = (int64_t)1 << 62;      // begin + n in the random order

}  // namespace

extern "C" {

int nerf_grid_dataset_batch(nerf_ctx* c, const nerf_grid_dataset_batch_args* a) {
    const char* fn = "nerf_grid_dataset_batch";
    int rc = require_ctx(fn, c);
    if (rc != NERF_OK) return rc;
    NERF_CHECK_STRUCT(fn, a, nerf_grid_dataset_batch_args);
    if (a->n_images < 1 || a->n_images > kDatasetMaxImages) {
        set_error("%s: n_images = %d must be in [1, 2^20]", fn, a->n_images);
        return NERF_E_INVALID;
    }
    if (a->height < 1 || a->height > kDatasetMaxSide || a->width < 1 || a->width > kDatasetMaxSide) {
        set_error("%s: height = %d and width = %d must be in [1, 2^15]", fn, a->height, a->width);
        return NERF_E_INVALID;
    }
    if (a->channels != 3 && a->channels != 4) {
        set_error("%s: channels = %d must be 3 or 4", fn, a->channels);
        return NERF_E_INVALID;
    }
    if (a->factor < 1 || a->factor > a->height || a->factor > a->width) {
        set_error("%s: factor = %d must be in [1, min(height, width)] = [1, %d]", fn, a->factor,
                  a->height < a->width ? a->height : a->width);
        return NERF_E_INVALID;
    }
    if (a->order != NERF_GRID_ORDER_IDENTITY && a->order != NERF_GRID_ORDER_PERMUTED && a->order != NERF_GRID_ORDER_RANDOM) {
        set_error("%s: order = %d must be NERF_GRID_ORDER_IDENTITY, _PERMUTED or _RANDOM", fn, a->order);
        return NERF_E_INVALID;
    }
    if (!(a->fx > 0.0) || !(a->fy > 0.0) || !std::isfinite(a->fx) || !std::isfinite(a->fy) || !std::isfinite(a->cx) ||
        !std::isfinite(a->cy)) {
        set_error("%s: fx = %g and fy = %g must be positive and finite, cx = %g and cy = %g finite", fn, a->fx, a->fy, a->cx, a->cy);
        return NERF_E_INVALID;
    }
    bool ndc = false;
    rc = check_ndc_coeffs(fn, a->ndc_coeffs, &ndc);
    if (rc != NERF_OK) return rc;
    GridDatasetBatch b{};
    b.height = a->height;
    b.width = a->width;
    b.channels = a->channels;
    b.h = a->height / a->factor;
    b.w = a->width / a->factor;
    b.n_rays = (int64_t)a->n_images * b.h * b.w;
    if (a->n < 0 || a->n > kGridMaxItems) {
        set_error("%s: n = %lld must be in [0, 2^26]", fn, (long long)a->n);
        return NERF_E_INVALID;
    }
    const int64_t last = a->order == NERF_GRID_ORDER_RANDOM ? kDatasetMaxRow : b.n_rays;
    if (a->begin < 0 || a->begin > last || a->n > last - a->begin) {
        set_error("%s: rows [begin, begin + n) = [%lld, %lld) must lie in [0, %lld]%s", fn, (long long)a->begin,
                  (long long)(a->begin + a->n), (long long)last,
                  a->order == NERF_GRID_ORDER_RANDOM ? "" : ", the rays of an epoch (n_images * (height / factor) * (width / factor))");
        return NERF_E_INVALID;
    }
    if (a->n > 0 && (!a->images || !a->c2w || !a->origins || !a->dirs || !a->rgb)) {
        set_error("%s: images, c2w, origins, dirs and rgb are required", fn);
        return NERF_E_INVALID;
    }
    if (a->channels == 4 && ((uintptr_t)a->images & 3u)) {
        set_error("%s: images must be 4-byte aligned when channels = 4", fn);
        return NERF_E_INVALID;
    }
    b.images = a->images;
    b.c2w = a->c2w;
    // svox2's Intrin.scale(1 / true_factor) in fp64, rounded where it meets the fp32 pixel coordinates
    const double s = 1.0 / ((double)a->height / (double)b.h);
    b.fx = (float)(a->fx * s);
    b.fy = (float)(a->fy * s);
    b.cx = (float)(a->cx * s);
    b.cy = (float)(a->cy * s);
    if (!(b.fx > 0.0f) || !(b.fy > 0.0f) || !std::isfinite(b.fx) || !std::isfinite(b.fy) || !std::isfinite(b.cx) || !std::isfinite(b.cy)) {
        set_error("%s: the scaled intrinsics (%g, %g, %g, %g) leave the range of fp32", fn, a->fx * s, a->fy * s, a->cx * s, a->cy * s);
        return NERF_E_INVALID;
    }
    b.white_bkgd = a->white_bkgd ? 1 : 0;
    b.factor = a->factor;
    b.order = a->order;
    const uint32_t klo = (uint32_t)(a->key & 0xffffffffull), khi = (uint32_t)(a->key >> 32);
    for (int r = 0; r < kDatasetRounds; ++r) b.rk[r] = hash32(hash32(klo + (uint32_t)r * 0x9e3779b9u) ^ khi);
    int bits = 2;
    while (((int64_t)1 << bits) < b.n_rays) bits += 2;
    b.half = bits / 2;
    b.begin = a->begin;
    b.n = a->n;
    b.origins = a->origins;
    b.dirs = a->dirs;
    b.rgb = a->rgb;
    b.indices = a->indices;
    b.ndc[0] = ndc ? a->ndc_coeffs[0] : 0.0f;
    b.ndc[1] = ndc ? a->ndc_coeffs[1] : 0.0f;
    if (a->n == 0) return NERF_OK;
    // ---- from here on the context is read ----
    DeviceGuard dg(c->device);
    HIP_TRY(launch_grid_dataset_batch(b, (hipStream_t)a->stream));
    return NERF_OK;
}

}  // extern "C"
