// PlenOctree (nerf_mi355x.h, "PlenOctree"): what octree_api.cpp and octree_kernels.hip share.
#pragma once
#include "grid_internal.h"

namespace nerf {

constexpr int kOctreeMaxIters = 1 << 16;                  // passes of one ray's march loop, at the latest
constexpr int64_t kOctreeMaxNodes = (int64_t)1 << 27;     // 8 cells each: cell indices stay below 2^30

// the tree as the kernels see it (passed by value)
struct OctreeDev {
    const int32_t* child;              // [n, 8]
    const float* data;                 // [n, 8, D]
    int64_t n_nodes;
    int32_t data_dim, basis_dim, max_depth, act;
    float invradius[3], offset[3];
    const int2* table;                 // nerf_octree_accelerate: [(2^table_levels)^3] (cell index, its depth), or nullptr
    int32_t table_levels;
};

struct OctreeRenderOpt {
    float step_size, sigma_thresh, stop_thresh, background_brightness;
};

struct OctreeRender {
    const float* origins;              // nullptr: the rays of `cam`
    const float* dirs;
    GridCam cam;
    int64_t n_rays;
    float* rgb;
    int32_t* steps;                    // or nullptr
    unsigned long long* capped;        // or nullptr
};

// the backward of a march ("PlenOctree: backward"): rays as OctreeRender's; exactly one of grad_rgb and rgb_gt
struct OctreeBackward {
    const float* origins;              // nullptr: the rays of `cam`
    const float* dirs;
    GridCam cam;
    int64_t n_rays;
    const float* grad_rgb;             // [n, 3], or nullptr: the fused loss form
    const float* rgb_gt;               // [n, 3], or nullptr
    float loss_scale;
    float* grad_data;                  // [n_nodes, 8, D], added to
    float* loss;                       // [1], added to, or nullptr
    float* rgb;                        // [n, 3] out, or nullptr
    unsigned long long* capped;        // or nullptr
};

// the workspace of a build from a grid of side 2^levels: byte offsets, needs no device. Level l (1 <= l < levels) has
// (2^l)^3 cells; occ[l] says whether a kept node lies under a cell, rank[l] is its rank among the occupied cells of its level
// (compact_device.h) or -1. counts[l] = occupied cells of level l = nodes of depth l; base[l] = index of the first of them.
struct OctreeBuildLayout {
    int levels;
    size_t occ[11], rank[11];          // by level; [0] unused
    size_t counts, base, block_offsets, total;
};
void octree_build_layout(int levels, OctreeBuildLayout* l);

struct OctreeBuild {
    const int32_t* links;              // the grid's
    const float* density;
    const float* sh;
    int32_t basis_dim, levels;
    char* ws;
    OctreeBuildLayout lay;
    int32_t* child;
    int32_t* parent_depth;
    float* data;
    int64_t n_nodes;                   // of the filling call: nothing is written past it
};

// *out (device) = 1 if an entry of child is negative or points at or past n_nodes, else 0
hipError_t launch_octree_check_child(const int32_t* child, int64_t n_nodes, int* out, hipStream_t s);
hipError_t launch_octree_render(const OctreeDev& t, const OctreeRenderOpt& o, const OctreeRender& r, hipStream_t s);
hipError_t launch_octree_backward(const OctreeDev& t, const OctreeRenderOpt& o, const OctreeBackward& b, hipStream_t s);
// table[(x, y, z)] of side 2^levels, 1 <= levels <= max_depth: the deepest cell of depth <= levels that holds the table cell
hipError_t launch_octree_table(const OctreeDev& t, int levels, int2* table, hipStream_t s);
// pyramid, one compaction per level, the bases; ws + lay.base[levels] (int32) is the node count
hipError_t launch_octree_plan(const OctreeBuild& b, hipStream_t s);
hipError_t launch_octree_fill(const OctreeBuild& b, hipStream_t s);

}  // namespace nerf

struct nerf_octree {
    nerf_ctx* ctx = nullptr;
    nerf::OctreeDev t{};
    int2* d_table = nullptr;           // owned; t.table
};
