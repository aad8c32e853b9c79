// Sparse voxel grid: floater views (nerf_mi355x.h, "Sparse voxel grid: floater views") - what grid_floater_api.cpp and
// grid_floater_kernels.hip share.
#pragma once
#include "grid_internal.h"

namespace nerf {

// the scan both views share (passed by value)
struct GridFloaterView {
    const int32_t* labels;             // [X, Y, Z]
    const int32_t* table;              // [n_labels + 1], 0 = ignore
    int64_t n_labels, nodes;
    int32_t size[3];
    float radius[3], center[3];
    float w2c[12];
    float fx, fy, cx, cy;              // the camera's, rounded to fp32
    int32_t width, height;             // the camera's
};

constexpr int kFloaterCounterSlots = 256;   // NERF_GRID_FLOATER_COUNTER_INTS = slots * stride
constexpr int kFloaterSlotStride = 32;      // int32 per slot: one 128-byte line each

struct GridFloaterHeat {
    int32_t use_density;               // min_density > 0
    float min_density;
    const float* depth;                // [height, width] of the camera, or nullptr: no occlusion test
    int32_t out_width, out_height;
    int32_t* counts;                   // [out_height, out_width]
    int32_t* counters;                 // [3]: dense, in_view, visible
    int32_t* counter_slots;            // [kFloaterCounterSlots * kFloaterSlotStride] workspace: the counters before they are added up
    float* heatmap;                    // [out_height, out_width]
};

hipError_t launch_grid_floater_heatmap(const GridDev& g, const GridFloaterView& v, const GridFloaterHeat& h, hipStream_t s);
hipError_t launch_grid_component_view(const GridFloaterView& v, unsigned long long* keys, int32_t* slots, hipStream_t s);

}  // namespace nerf
