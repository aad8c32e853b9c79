// Sparse voxel grid: background layers (svox2's multi-sphere image, forward side) and their thinning.
// Semantics: include/nerf_mi355x.h, "Sparse voxel grid: background layers". Design and measurements: DESIGN.md section 7l.
//
// Mapping: one lane per ray. The pass runs after the foreground on its colour and log_transmit; a lane sets its ray up with
// setup_ray of grid_device.h (the foreground's o, d, delta_scale and miss rule, bit for bit), walks the n sphere radii alone
// and writes its ray's colour and log_transmit back. A texel's 4 channels are one 16-byte load and the two layers of a
// corner are 32 contiguous bytes, so a step is 4 link loads and 8 float4 loads, all channels interpolated from the same
// registers (the reference runs four scalar trilinear fetches per step, sigma and then each colour). Rows reach
// capacity * nlayers * 4 floats, past 2^31 at 2048 x 1024 texels of 64 layers: every row index is int64_t.
// The march itself (set-up, sphere hit, texel coordinates, fetch, stop rule) is background_march of grid_background_device.h,
// which the taped pass and the backward of grid_background_train_kernels.hip walk too.
// The image form makes its rays in the launch and, like grid_depth_kernels.hip, gives a wavefront an 8 x 8 tile of pixels
// rather than 64 pixels of a row: neighbouring rays hit neighbouring texels on every sphere, so a tile's 64 loads fall on
// fewer lines than a row's (DESIGN.md has the A/B). No LDS, no scratch, no atomics, no shuffles: a result depends on its own
// ray only, two runs give the same bits.
#include "grid_background_device.h"

namespace nerf {
namespace {

constexpr int kTile = 8;      // pixels per side of a wavefront's tile: kTile * kTile = 64 lanes

// the pixel of this thread in row-major order, or -1 outside the image
__device__ __forceinline__ int64_t background_pixel(const GridCam& cam) {
    const int64_t tid = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    const int64_t tile = tid / (kTile * kTile);
    const int lane = (int)(tid % (kTile * kTile));
    const int tiles_x = (cam.width + kTile - 1) / kTile;
    const int64_t px = (tile % tiles_x) * kTile + lane % kTile;
    const int64_t py = (tile / tiles_x) * kTile + lane / kTile;
    return px < cam.width && py < cam.height ? py * cam.width + px : -1;
}

int64_t background_image_threads(const GridCam& cam) {
    return (int64_t)((cam.width + kTile - 1) / kTile) * ((cam.height + kTile - 1) / kTile) * (kTile * kTile);
}

template <bool IMAGE>
__global__ __launch_bounds__(kGridThreads) void grid_background_kernel(GridDev g, GridBg bg, GridRenderOpt opt, GridBgRender r) {
    int64_t ray;
    GridRay rs;
    if (IMAGE) {
        ray = background_pixel(r.cam);
        if (ray < 0) return;
        camera_ray(r.cam, ray, rs.o, rs.d);
    } else {
        ray = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
        if (ray >= r.n_rays) return;
        load_ray(r.origins, r.dirs, ray, rs);
    }
    float log_t = r.log_transmit[ray];
    if (log_t < -25.0f) return;      // left alone: no layers, no brightness term
    setup_ray<false>(g, opt, rs);
    float* rgb = r.rgb + ray * 3;
    if (!rs.ok) {
        const float b = mul(expf(log_t), opt.background_brightness);
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[c] = add(rgb[c], b);
        return;
    }

    float out[3] = {0.0f, 0.0f, 0.0f};
    log_t = background_march(g, bg, opt, rs, log_t, [&](const BgSample&, const float4& v, float, float weight, float) {
        out[0] = add(out[0], mul(weight, fmaxf(background_colour(v.x), 0.0f)));
        out[1] = add(out[1], mul(weight, fmaxf(background_colour(v.y), 0.0f)));
        out[2] = add(out[2], mul(weight, fmaxf(background_colour(v.z), 0.0f)));
    });
    const float b = mul(expf(log_t), opt.background_brightness);
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[c] = add(rgb[c], add(out[c], b));
    r.log_transmit[ray] = log_t;
}

// ---- thinning -------------------------------------------------------------------------------------------------------------
// one thread per (texel, layer): the texel has a row and its sigma in that layer is >= the threshold
__global__ __launch_bounds__(kGridThreads) void background_mask_kernel(GridBg bg, float sigma_thresh, uint8_t* __restrict__ mask) {
    const int64_t n = (int64_t)2 * bg.reso * bg.reso * bg.nlayers;
    const int64_t idx = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (idx >= n) return;
    const int64_t texel = idx / bg.nlayers;
    const int layer = (int)(idx % bg.nlayers);
    const int link = bg.links[texel];
    uint8_t m = 0;
    if (link >= 0 && (int64_t)link < bg.capacity) m = bg.data[((int64_t)link * bg.nlayers + layer) * 4 + 3] >= sigma_thresh ? 1 : 0;
    mask[idx] = m;
}

// one thread per texel: it has a row and any byte of its column of the (dilated) mask is set
__global__ __launch_bounds__(kGridThreads) void background_keep_kernel(GridBg bg, const uint8_t* __restrict__ mask,
                                                                        uint8_t* __restrict__ keep) {
    const int64_t n = (int64_t)2 * bg.reso * bg.reso;
    const int64_t texel = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (texel >= n) return;
    const int link = bg.links[texel];
    uint8_t any = 0;
    if (link >= 0 && (int64_t)link < bg.capacity)
        for (int z = 0; z < bg.nlayers; ++z) any |= mask[texel * bg.nlayers + z];
    keep[texel] = any ? 1 : 0;
}

// one thread per float4 of the new table: row new_links[texel] <- row links[texel]
__global__ __launch_bounds__(kGridThreads) void background_gather_kernel(GridBg bg, const int32_t* __restrict__ new_links,
                                                                          int64_t new_capacity, float4* __restrict__ new_data) {
    const int64_t n = (int64_t)2 * bg.reso * bg.reso * bg.nlayers;
    const int64_t idx = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (idx >= n) return;
    const int64_t texel = idx / bg.nlayers;
    const int layer = (int)(idx % bg.nlayers);
    const int dst = new_links[texel], src = bg.links[texel];
    if (dst < 0 || (int64_t)dst >= new_capacity || src < 0 || (int64_t)src >= bg.capacity) return;
    new_data[(int64_t)dst * bg.nlayers + layer] = reinterpret_cast<const float4*>(bg.data)[(int64_t)src * bg.nlayers + layer];
}

}  // namespace

hipError_t launch_grid_background(const GridDev& g, const GridBg& bg, const GridRenderOpt& o, const GridBgRender& r, hipStream_t s) {
    if (r.n_rays <= 0) return hipSuccess;
    if (r.origins == nullptr)
        grid_background_kernel<true><<<blocks_for(background_image_threads(r.cam)), kGridThreads, 0, s>>>(g, bg, o, r);
    else
        grid_background_kernel<false><<<blocks_for(r.n_rays), kGridThreads, 0, s>>>(g, bg, o, r);
    return hipGetLastError();
}

hipError_t launch_grid_background_plan(const GridBgSparsify& a, hipStream_t s) {
    const int32_t size[3] = {2 * a.bg.reso, a.bg.reso, a.bg.nlayers};
    const int64_t texels = (int64_t)size[0] * size[1], n = texels * size[2];
    uint8_t* cur = a.mask;
    uint8_t* other = a.mask + n;
    background_mask_kernel<<<blocks_for(n), kGridThreads, 0, s>>>(a.bg, a.sigma_thresh, cur);
    hipError_t e = hipGetLastError();
    for (int k = 0; k < a.dilate && e == hipSuccess; ++k) {
        e = launch_grid_dilate(cur, size, other, s);
        uint8_t* t = cur;
        cur = other;
        other = t;
    }
    if (e != hipSuccess) return e;
    background_keep_kernel<<<blocks_for(texels), kGridThreads, 0, s>>>(a.bg, cur, a.keep);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_grid_compact(a.keep, texels, a.block_offsets, a.new_links, a.count, s);
}

hipError_t launch_grid_background_gather(const GridBg& bg, const int32_t* new_links, int64_t new_capacity, float* new_data,
                                         hipStream_t s) {
    const int64_t n = (int64_t)2 * bg.reso * bg.reso * bg.nlayers;
    background_gather_kernel<<<blocks_for(n), kGridThreads, 0, s>>>(bg, new_links, new_capacity, reinterpret_cast<float4*>(new_data));
    return hipGetLastError();
}

}  // namespace nerf
