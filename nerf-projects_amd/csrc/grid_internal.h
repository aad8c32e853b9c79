// Sparse voxel grid (nerf_mi355x.h, "Sparse voxel grid"): what the host and the device side of the grid share.
//   grid_api.cpp            create / render / sample / accelerate, and the argument checks every grid_*_api.cpp uses (below)
//   grid_train_api.cpp      fused backward, TV gradient, optimiser step; the same with the loss terms and the edge rule
//   grid_autograd_api.cpp   taped render, render backward with a caller's cotangent (and with the loss terms), sample backward
//   grid_resample_api.cpp   lattice density, weight render, threshold, dilate, compact, gather
//   grid_components_api.cpp occupancy, labelling, volumes, keep mask, row copy
//   grid_depth_api.cpp      expected depth, threshold depth, ray length
//   grid_depth_autograd_api.cpp   taped expected depth, backward with cotangents for depth and log_transmit
//   grid_regularisers_api.cpp     total variation and the sparsity term as values, and their backwards
//   grid_half_api.cpp       half-precision colours: pack / unpack, create; render and sample are dispatched from grid_api.cpp
//   grid_palette_api.cpp    palette-quantised colours: the median cut, create; render and sample likewise
//   grid_background_api.cpp background layers: attach / detach, the background pass, the two calls of the thinning
//   grid_background_train_api.cpp   background layers, training: taped pass, backward, TV gradient, optimiser step
//   grid_dataset_api.cpp    training data: a batch of rays from the resident images (takes a context, no grid)
//   grid_ndc_kernels.hip    the NDC warp on a caller's rays (its entry point, nerf_grid_rays_to_ndc, is in grid_api.cpp)
//   grid_mesh_api.cpp       surface meshes: marching cubes on the grid's own lattice, normals and colours at points
//   grid_*_kernels.hip      the kernels of each, on grid_device.h (sampling, rays) and compact_device.h (compaction)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "nerf_mi355x.h"

struct nerf_ctx;

namespace nerf {

constexpr int kGridSkipCap = 32;       // largest stored skip value: a distance of 31 cells
constexpr float kGridSkipMaxT = 131072.0f;      // 2^17: the range of |origin| and |t| (grid units) in which skip data is used
constexpr int64_t kGridMaxItems = (int64_t)1 << 26;   // rays / points / nodes per call: 32 lanes each stay inside one launch

// the grid as the kernels see it (passed by value)
struct GridDev {
    const int32_t* links;
    const float* density;
    const float* sh;                   // [capacity, 3 B], or nullptr on a half-precision grid
    const uint16_t* sh_half;           // [capacity, grid_half_row_halfs(B)] packed fp16 rows (grid_half_kernels.hip), or nullptr
    const uint8_t* skip;               // [X, Y, Z] bytes indexed like links (base cell = its lowest node), or nullptr
    int32_t size[3];
    int32_t basis_dim;
    int64_t capacity;
    // world2grid of the reference, fp32, each operation rounded: _offset = 0.5 (1 - center / radius), _scaling = 0.5 / radius,
    // offset = _offset * size - 0.5, scaling = _scaling * size
    float offset[3], scaling[3];
};

struct GridRenderOpt {
    float step_size, sigma_thresh, stop_thresh, background_brightness, near_clip;
};

struct GridCam {
    double c2w[12];
    double fx, fy, cx, cy;
    int32_t width, height;
    float ndc[2];                      // ndc_coeffs; ndc[0] <= 0: a plain pinhole camera (camera_ray, grid_device.h)
};

struct GridRender {
    const float* origins;              // nullptr: the rays of `cam`
    const float* dirs;
    GridCam cam;
    int64_t n_rays;
    float* rgb;
    float* log_transmit;
    unsigned long long* counters;
};

// ---- training (grid_train_kernels.hip) ----
struct GridFused {
    const float* origins;
    const float* dirs;
    const float* rgb_gt;
    int64_t n_rays;
    float grad_scale;                  // 2 / (3 n_rays)
    float* rgb;
    float* log_transmit;               // or nullptr
    float* grad_density;               // [capacity, 1], added to
    float* grad_sh;                    // [capacity, 3 B], added to
    uint8_t* mask;                     // [capacity], 1 stored at every kept corner of every shaded sample
    float beta_loss, sparsity_loss;    // read by the LOSSES instantiations only (grid_train_losses_kernels.hip)
};

struct GridTv {
    const float* data;                 // the table differentiated: [capacity, cols]
    float* grad;
    uint8_t* mask;
    int64_t start, count;              // cells (start + i) mod X Y Z, i < count
    int32_t cols, start_dim, end_dim;
    float scale;
    float axis_scale[3];               // reso / 256
};

struct GridOptim {
    float* data;
    float* rms;                        // RMSProp only
    const float* grad;
    const uint8_t* mask;
    int64_t rows;
    int32_t cols;
    float beta, lr, eps, minval;
};

hipError_t launch_grid_fused(const GridDev& g, const GridRenderOpt& o, const GridFused& r, hipStream_t s);
hipError_t launch_grid_tv_grad(const GridDev& g, const GridTv& a, hipStream_t s);
hipError_t launch_grid_optim_step(const GridOptim& a, int rmsprop, hipStream_t s);
// grid_train_losses_kernels.hip: the same kernels (grid_train_device.h) with the loss terms / the edge rule compiled in
hipError_t launch_grid_fused_losses(const GridDev& g, const GridRenderOpt& o, const GridFused& r, hipStream_t s);
hipError_t launch_grid_tv_grad_edge(const GridDev& g, const GridTv& a, hipStream_t s);

// ---- gradients for autograd (grid_autograd_kernels.hip) ----
struct GridTaped {
    const float* origins;
    const float* dirs;
    int64_t n_rays;
    float* rgb;
    float* log_transmit;               // or nullptr
    double* tape;                      // [n_rays, 3]: the colour as the fp64 sum of its exact terms
};

struct GridRenderBwd {
    const float* origins;
    const float* dirs;
    int64_t n_rays;
    const float* grad_rgb;             // [n_rays, 3]
    const double* tape;
    float* grad_density;               // added to; each of the three may be nullptr: nothing is issued for it
    float* grad_sh;
    uint8_t* mask;
    // read by the LOSSES instantiations only (grid_train_losses_kernels.hip)
    const float* log_transmit;         // [n_rays] the taped render's; may be nullptr where beta_loss is 0
    float beta_loss, sparsity_loss;
};

struct GridSampleBwd {
    const float* points;
    int64_t n;
    int32_t grid_coords, want_colors;
    const float* grad_out_density;     // [n, 1]
    const float* grad_out_sh;          // [n, 3 B]
    float* grad_density;               // added to, or nullptr
    float* grad_sh;
};

hipError_t launch_grid_render_taped(const GridDev& g, const GridRenderOpt& o, const GridTaped& r, hipStream_t s);
hipError_t launch_grid_render_bwd(const GridDev& g, const GridRenderOpt& o, const GridRenderBwd& r, hipStream_t s);
hipError_t launch_grid_sample_bwd(const GridDev& g, const GridSampleBwd& a, hipStream_t s);
hipError_t launch_grid_render_bwd_losses(const GridDev& g, const GridRenderOpt& o, const GridRenderBwd& r, hipStream_t s);

// ---- resampling (grid_resample_kernels.hip) ----
constexpr int64_t kGridMaxLattice = (int64_t)1 << 30;   // nodes of a resampling lattice: 1024^3

struct GridLattice {
    const float* axis[3];              // node coordinates per axis, in the old grid's coordinates
    int32_t size[3];
    float* density;                    // [X', Y', Z']
};

struct GridWeight {
    GridCam cam;
    const float* density;              // [X', Y', Z'] dense
    float* max_weight;                 // [X', Y', Z'], raised
    int32_t size[3];
    float offset[3], scaling[3];       // world2grid of the lattice (grid_world2grid)
    float step_size, stop_thresh;
};

struct GridGather {
    const float* axis[3];
    int32_t size[3];
    const int32_t* links;              // [X', Y', Z'] of the new grid
    const float* lattice_density;
    int32_t* node_of_row;              // [rows] workspace
    int64_t rows;
    float* density_data;               // [rows, 1]
    float* sh_data;                    // [rows, 3 B]
};

hipError_t launch_grid_lattice_density(const GridDev& g, const GridLattice& a, hipStream_t s);
hipError_t launch_grid_weight_render(const GridWeight& a, hipStream_t s);
hipError_t launch_grid_threshold(const float* volume, int64_t n, float threshold, uint8_t* mask, hipStream_t s);
hipError_t launch_grid_dilate(const uint8_t* in, const int32_t size[3], uint8_t* out, hipStream_t s);
// block_offsets: [compact_blocks(n)] workspace (compact_device.h)
hipError_t launch_grid_compact(const uint8_t* mask, int64_t n, int32_t* block_offsets, int32_t* links, int32_t* count,
                               hipStream_t s);
hipError_t launch_grid_gather(const GridDev& g, const GridGather& a, hipStream_t s);

// ---- connected components (grid_components_kernels.hip) ----
struct GridLabel {
    const uint8_t* occ;                // [X, Y, Z] bytes 0 / 1
    int32_t size[3];
    int32_t connectivity;              // 6, 18 or 26
    int32_t* parent;                   // [X, Y, Z] workspace
    int32_t* block_offsets;            // [compact_blocks(X Y Z)] workspace (compact_device.h)
    int32_t* labels;                   // [X, Y, Z]
    int32_t* status;                   // [2]: the component count, the error word
};

struct GridCopyRows {
    const int32_t* old_links;          // [X, Y, Z]
    const int32_t* new_links;          // [X, Y, Z]: -1 or a running index over a subset of the old kept nodes
    int64_t nodes, old_rows, new_rows;
    int32_t cols;                      // of sh
    const float* old_density;
    const float* old_sh;
    int32_t* src_row;                  // [new_rows] workspace
    float* density;                    // [new_rows, 1]
    float* sh;                         // [new_rows, cols]
};

hipError_t launch_grid_occupancy(const GridDev& g, int use_density, float threshold, uint8_t* occ, hipStream_t s);
hipError_t launch_grid_label(const GridLabel& a, hipStream_t s);
hipError_t launch_grid_label_volumes(const int32_t* labels, int64_t n, int64_t count, int32_t* volumes, hipStream_t s);
hipError_t launch_grid_keep_mask(const int32_t* links, const int32_t* labels, int64_t n, const uint8_t* floater, int64_t count,
                                 uint8_t* mask, hipStream_t s);
hipError_t launch_grid_copy_rows(const GridCopyRows& a, hipStream_t s);

// ---- depth and ray lengths (grid_depth_kernels.hip) ----
struct GridDepth {
    const float* origins;              // nullptr: the rays of `cam`
    const float* dirs;
    GridCam cam;
    int64_t n_rays;
    int32_t mode;                      // NERF_GRID_DEPTH_*
    float sigma_thresh;                // of the threshold mode
    float* depth;                      // [n_rays]
    float* log_transmit;               // [n_rays] or nullptr (expected mode)
};

hipError_t launch_grid_depth(const GridDev& g, const GridRenderOpt& o, const GridDepth& r, hipStream_t s);

// ---- gradients of depth and log_transmit (grid_depth_autograd_kernels.hip) ----
struct GridDepthTaped {
    const float* origins;
    const float* dirs;
    int64_t n_rays;
    float* depth;                      // [n_rays]
    float* log_transmit;               // or nullptr
    double* tape;                      // [n_rays]: the depth as the fp64 sum of its fp32 terms
};

struct GridDepthBwd {
    const float* origins;
    const float* dirs;
    int64_t n_rays;
    const float* grad_depth;           // [n_rays] or nullptr
    const float* grad_log_transmit;    // [n_rays] or nullptr
    const double* tape;                // nullptr iff grad_depth is
    float* grad_density;               // [capacity, 1], added to
};

hipError_t launch_grid_depth_taped(const GridDev& g, const GridRenderOpt& o, const GridDepthTaped& r, hipStream_t s);
hipError_t launch_grid_depth_bwd(const GridDev& g, const GridRenderOpt& o, const GridDepthBwd& r, hipStream_t s);

// ---- regularisers as values (grid_regularisers_kernels.hip) ----
constexpr int kGridTvValueItems = 256;   // items (cell, column) per workgroup = per fp64 partial

struct GridTvValue {
    const float* data;                 // the table: [capacity, cols]
    int32_t cols, start_dim, end_dim;
    int32_t edge;                      // svox2's ignore_edge
    const void* cells;                 // [count] flat node indices, or nullptr: the (X-1)(Y-1)(Z-1) cells in C order
    int32_t cells_int64;
    int64_t count;                     // cells of the call: the divisor
    float axis_scale[3];               // reso / 256
    double* partials;                  // forward: one per workgroup
    float* value;                      // forward: [1]
    const float* grad_value;           // backward: [1]
    float* grad;                       // backward: [capacity, cols], added to
};

struct GridSparsity {
    const float* origins;
    const float* dirs;
    int64_t n_rays;
    float* sparsity;                   // forward: [n_rays]
    const float* grad_sparsity;        // backward: [n_rays]
    float* grad_density;               // backward: [capacity, 1], added to
};

hipError_t launch_grid_tv_value(const GridDev& g, const GridTvValue& a, hipStream_t s);
hipError_t launch_grid_tv_value_bwd(const GridDev& g, const GridTvValue& a, hipStream_t s);
hipError_t launch_grid_sparsity(const GridDev& g, const GridRenderOpt& o, const GridSparsity& r, hipStream_t s);
hipError_t launch_grid_sparsity_bwd(const GridDev& g, const GridRenderOpt& o, const GridSparsity& r, hipStream_t s);

// ---- argument checks (grid_api.cpp): NERF_OK, or NERF_E_INVALID with last_error set. None needs a device or reads a handle. ----
void set_error(const char* fmt, ...);
int require_ctx(const char* fn, const nerf_ctx* c);                      // "NULL context"
int require_grid(const char* fn, const nerf_sparse_grid* grid);          // "NULL grid"
// for the entry points that read or write an fp32 SH table through the handle: a grid of nerf_grid_create_half or of
// nerf_grid_create_palette is refused
int refuse_half_grid(const char* fn, const nerf_sparse_grid* grid);
// for every training, autograd, resampling and TV entry point, also those that read density only: a grid of
// nerf_grid_create_palette is refused
int refuse_palette_grid(const char* fn, const nerf_sparse_grid* grid);
// the link check of nerf_grid_create / nerf_grid_create_half: synchronises `s`; NERF_E_INVALID for a link >= capacity
int check_grid_links(const char* fn, const int32_t* links, int64_t n, int64_t capacity, hipStream_t s);
// reso not NULL, every side in [2, 1024] (so that a cell exists on every axis), at most 2^30 nodes
int check_grid_reso(const char* fn, const int32_t* reso, int64_t* nodes);
// ndc_coeffs of a public struct: NERF_OK and *use = whether NDC is on ([0] > 0); NaN, infinity or [0] > 0 with [1] <= 0 refused
int check_ndc_coeffs(const char* fn, const float ndc_coeffs[2], bool* use);
// for the entry points in which an NDC camera has no meaning (`why` ends the message)
int refuse_ndc_camera(const char* fn, const GridCam& cam, const char* why);
// a public camera (struct_size, size, intrinsics, ndc_coeffs) / the public render options (struct_size, what is not built, ranges), converted
int check_grid_camera(const char* fn, const nerf_grid_camera* cam, GridCam* out);
int check_grid_options(const char* fn, const nerf_grid_render_options* o, GridRenderOpt* out);

// world2grid of the reference (svox2.py:411-412, 1504-1506: fp32 tensors, each operation rounded; compiled with
// -ffp-contract=off) after the check that radius is positive and finite and center finite: GridDev::offset / scaling
inline int grid_world2grid(const char* fn, const float center[3], const float radius[3], const int32_t reso[3], float offset[3],
                           float scaling[3]) {
    for (int k = 0; k < 3; ++k) {
        if (!(radius[k] > 0.0f) || !std::isfinite(radius[k]) || !std::isfinite(center[k])) {
            set_error("%s: axis %d: radius = %g must be positive and finite, center = %g finite", fn, k, radius[k], center[k]);
            return NERF_E_INVALID;
        }
        const float ratio = center[k] / radius[k];
        const float one_minus = 1.0f - ratio;
        const float off = 0.5f * one_minus;
        const float scl = 0.5f / radius[k];
        const float off_g = off * (float)reso[k];
        offset[k] = off_g - 0.5f;
        scaling[k] = scl * (float)reso[k];
    }
    return NERF_OK;
}

hipError_t launch_grid_render(const GridDev& g, const GridRenderOpt& o, const GridRender& r, hipStream_t s);
hipError_t launch_grid_gen_rays(const GridCam& cam, float* origins, float* dirs, hipStream_t s);
// rays_to_ndc (grid_device.h) on n rays, one lane each; an output may be its input
hipError_t launch_grid_rays_to_ndc(const float* origins, const float* dirs, int64_t n, float coeffx, float coeffy,
                                   float* origins_out, float* dirs_out, hipStream_t s);
hipError_t launch_grid_sample(const GridDev& g, const float* points, int64_t n, int grid_coords, int want_colors,
                              float* density, float* sh, hipStream_t s);
// skip [X * Y * Z] bytes: kGridSkipCap stream-ordered launches, no atomics
hipError_t launch_grid_accelerate(const GridDev& g, uint8_t* skip, hipStream_t s);
// *out (device) = 1 if any link is >= capacity, else 0
hipError_t launch_grid_check_links(const int32_t* links, int64_t n, int64_t capacity, int* out, hipStream_t s);
hipError_t launch_grid_project_sh(const float* raw, int64_t m, int n_dirs, int basis_dim, const float* P, float* sh_out,
                                  int64_t row0, hipStream_t s);

// ---- half-precision colours (grid_half_kernels.hip) ----
// One packed row: channel-major like sh_data, a channel in kGridHalfChannel slots (B rounded up to even, so that coefficients
// (2 j, 2 j + 1) of a channel share an aligned 32-bit word; 1 at B = 1), the row zero-padded to a power of two of halfs.
constexpr int grid_half_channel_halfs(int B) { return B == 1 ? 1 : (B + 1) / 2 * 2; }       // 10 / 4 / 1
constexpr int grid_half_row_halfs(int B) { return B == 9 ? 32 : (B == 4 ? 16 : 4); }        // 64 / 32 / 8 bytes

struct GridHalfPack {
    const float* sh;                   // [rows, 3 B]
    uint16_t* sh_half;                 // the whole packed table; rows [row0, row0 + rows) are written
    int64_t rows, row0;
    int32_t basis_dim;
    unsigned long long* clamped;       // += entries beyond +-65504, or nullptr
};

hipError_t launch_grid_pack_half(const GridHalfPack& a, hipStream_t s);
hipError_t launch_grid_unpack_half(const uint16_t* sh_half, int64_t rows, int basis_dim, float* sh, hipStream_t s);
// on a GridDev with sh_half: the half twins of launch_grid_render / launch_grid_sample (same arguments, same results as the
// fp32 kernels give on the widened table, bit for bit). pair: two coefficients per lane (NERF_GRID_HALF_LANES_PAIR), else one.
hipError_t launch_grid_half_render(const GridDev& g, const GridRenderOpt& o, const GridRender& r, bool pair, hipStream_t s);
hipError_t launch_grid_half_sample(const GridDev& g, const float* points, int64_t n, int grid_coords, int want_colors,
                                   float* density, float* sh, hipStream_t s);

// ---- palette-quantised colours (grid_palette_kernels.hip, grid_median_cut_kernels.hip) ----
// The colour tables of a palette grid; Q = basis_dim - retain. Passed to the palette kernels beside GridDev, whose sh and
// sh_half are nullptr on such a grid: GridDev, and with it the arguments of every other kernel, stays as it was.
struct GridPalette {
    const uint16_t* map;               // [capacity, Q] palette indices, node-major, rows not padded
    const uint16_t* colors;            // [Q, entries, 3] fp16
    const uint16_t* retained;          // [capacity, retain, 3] fp16
    int32_t retain, entries;           // entries = 2^bits
};

struct GridMedianCut {
    const float* colors;               // [m, 3]
    int64_t m;
    int32_t bits;
    uint16_t* ids;                     // [m]
    uint16_t* palette;                 // [2^bits, 3] fp16
    void* workspace;
};

// byte offsets into the workspace of a median cut, and its size; needs no device
struct GridMedianCutLayout {
    size_t keys, perm, minmax, minmax_bytes, nonfinite, sort, sort_bytes, total;
};
void grid_median_cut_layout(int64_t m, int bits, GridMedianCutLayout* l);
// fills the identity order and counts the rows with a non-finite component into workspace + l.nonfinite (uint64)
hipError_t launch_grid_median_cut_count(const GridMedianCut& a, const GridMedianCutLayout& l, hipStream_t s);
// the cut itself, after launch_grid_median_cut_count found nothing; hipErrorOutOfMemory if the sort wants more than l.sort_bytes
hipError_t launch_grid_median_cut(const GridMedianCut& a, const GridMedianCutLayout& l, hipStream_t s);
// the palette twins of launch_grid_render / launch_grid_sample: the results of the fp32 kernels on the dequantised table
hipError_t launch_grid_palette_render(const GridDev& g, const GridPalette& p, const GridRenderOpt& o, const GridRender& r,
                                      hipStream_t s);
hipError_t launch_grid_palette_sample(const GridDev& g, const GridPalette& p, const float* points, int64_t n, int grid_coords,
                                      int want_colors, float* density, float* sh, hipStream_t s);
// *out (device) = 1 if any of the n indices is >= entries, else 0
hipError_t launch_grid_palette_check(const uint16_t* map, int64_t n, int entries, int* out, hipStream_t s);

// ---- surface meshes (grid_mesh_kernels.hip; the extraction itself is mesh_kernels.hip's, nerf_internal.h) ----
struct GridMeshAttr {
    const float* points;               // [n, 3] grid coordinates
    int64_t n;
    const uint8_t* mask;               // [X, Y, Z] or nullptr
    int32_t color_mode;                // NERF_GRID_MESH_COLOR_*
    float view[3];                     // unit direction of NERF_GRID_MESH_COLOR_VIEW
    float* normals;                    // [n, 3] or nullptr
    float* colors;                     // [n, 3]; nullptr iff color_mode is NERF_GRID_MESH_COLOR_NONE
    int32_t half_channel, half_row;    // set by the launcher: the layout of a packed half row
};

// `p` is read on a palette grid only; half / palette say which colour table `g` carries
hipError_t launch_grid_mesh_attributes(const GridDev& g, const GridPalette& p, bool half, bool palette, const GridMeshAttr& a,
                                       hipStream_t s);

// ---- background layers (grid_background_kernels.hip) ----
struct GridBg {
    const int32_t* links;              // [2 reso, reso], or nullptr: no background attached
    const float* data;                 // [capacity, nlayers, 4]
    int32_t nlayers, reso;
    int64_t capacity;
};

struct GridBgRender {
    const float* origins;              // nullptr: the rays of `cam`
    const float* dirs;
    GridCam cam;
    int64_t n_rays;
    float* rgb;                        // [n_rays, 3] in / out
    float* log_transmit;               // [n_rays] in / out
};

struct GridBgSparsify {
    GridBg bg;
    float sigma_thresh;
    int32_t dilate;
    uint8_t* mask;                     // [2, 2 reso, reso, nlayers]
    uint8_t* keep;                     // [2 reso, reso]
    int32_t* block_offsets;
    int32_t* new_links;
    int32_t* count;
};

hipError_t launch_grid_background(const GridDev& g, const GridBg& bg, const GridRenderOpt& o, const GridBgRender& r, hipStream_t s);
hipError_t launch_grid_background_plan(const GridBgSparsify& a, hipStream_t s);
hipError_t launch_grid_background_gather(const GridBg& bg, const int32_t* new_links, int64_t new_capacity, float* new_data,
                                         hipStream_t s);

// ---- background layers, training (grid_background_train_kernels.hip) ----
struct GridBgTaped {
    const float* origins;
    const float* dirs;
    int64_t n_rays;
    float* rgb;                        // [n_rays, 3] in / out
    const float* log_transmit;         // [n_rays]: the foreground's
    float* log_transmit_out;           // [n_rays]
    double* tape;                      // [n_rays, 3] in / out
    double* tape_background;           // [n_rays, 3] out
};

struct GridBgBwd {
    const float* origins;
    const float* dirs;
    int64_t n_rays;
    const float* grad_rgb;             // [n_rays, 3]
    const float* log_transmit;         // [n_rays]: the foreground's
    const double* tape_background;     // [n_rays, 3]
    float* grad_background;            // [capacity, nlayers, 4], added to
    uint8_t* mask_background;          // [capacity, nlayers], or nullptr
};

struct GridBgTv {
    int64_t start, count;              // cells (start + i) mod 2R R L, i < count
    float scale_sigma, scale_color;
    float* grad;                       // [capacity, nlayers, 4], added to
    uint8_t* mask;                     // [capacity, nlayers]
};

struct GridBgOptim {
    float* data;                       // [rows, 4], rows = capacity * nlayers
    float* rms;                        // RMSProp only
    const float* grad;
    const uint8_t* mask;               // [rows]
    int64_t rows;
    float beta, lr_sigma, lr_color, eps, minval;
};

hipError_t launch_grid_background_taped(const GridDev& g, const GridBg& bg, const GridRenderOpt& o, const GridBgTaped& r, hipStream_t s);
hipError_t launch_grid_background_bwd(const GridDev& g, const GridBg& bg, const GridRenderOpt& o, const GridBgBwd& r, hipStream_t s);
hipError_t launch_grid_background_tv(const GridBg& bg, const GridBgTv& a, hipStream_t s);
hipError_t launch_grid_background_optim(const GridBgOptim& a, int rmsprop, hipStream_t s);

}  // namespace nerf

struct nerf_sparse_grid {
    nerf_ctx* ctx = nullptr;
    nerf::GridDev g{};
    uint8_t* d_skip = nullptr;
    bool half = false;                 // made by nerf_grid_create_half: g.sh_half is the colour table, g.sh is nullptr
    bool half_pair = false;            // ... and it renders with two coefficients per lane
    nerf::GridBg bg{};                 // nerf_grid_set_background; bg.links == nullptr: none
    bool palette = false;              // made by nerf_grid_create_palette: `pal` holds the colours, g.sh and g.sh_half are nullptr
    nerf::GridPalette pal{};
};
