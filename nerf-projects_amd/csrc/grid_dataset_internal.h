// Sparse voxel grid: training data (nerf_mi355x.h, "Sparse voxel grid: training data") - what grid_dataset_api.cpp and
// grid_dataset_kernels.hip share.
#pragma once
#include "grid_internal.h"

namespace nerf {

constexpr int kDatasetRounds = 4;      // Feistel rounds, and round keys

// the header's hash32: the round function on the device, the round keys on the host
__host__ __device__ inline uint32_t hash32(uint32_t v) {
    v ^= v >> 16;
    v *= 0x7feb352du;
    v ^= v >> 15;
    v *= 0x846ca68bu;
    v ^= v >> 16;
    return v;
}

// one batch (passed by value)
struct GridDatasetBatch {
    const uint8_t* images;             // [n_images, height, width, channels]
    const float* c2w;                  // [n_images, 12]
    int32_t height, width, channels;   // full resolution
    int32_t h, w;                      // height / factor, width / factor
    int64_t n_rays;                    // N = n_images * h * w
    float fx, fy, cx, cy;              // scaled by h / height, rounded to fp32
    int32_t white_bkgd, factor, order;
    uint32_t rk[kDatasetRounds];       // round keys of the epoch's key
    int32_t half;                      // bits of one Feistel half
    int64_t begin, n;
    float* origins;
    float* dirs;
    float* rgb;
    int64_t* indices;                  // or nullptr
    float ndc[2];                      // ndc_coeffs; ndc[0] <= 0: world rays
};

hipError_t launch_grid_dataset_batch(const GridDatasetBatch& b, hipStream_t s);

}  // namespace nerf
