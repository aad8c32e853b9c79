// Sparse voxel grid, surface meshes: normals and colours at points of the lattice (nerf_grid_mesh_attributes). Semantics:
// include/nerf_mi355x.h, "Sparse voxel grid: surface meshes". The geometry itself (nerf_grid_marching_cubes) is
// mesh_kernels.hip's passes with the grid as the source of the node values.
//
// One thread per point. A point's cell and weights are grid_device.h's point_cell - the sampler's - so its SH row is, bit for
// bit, what nerf_grid_sample returns there: the 8 corner links (load_links), one coefficient fetched per corner (from the fp32
// table, or through grid_fetch_device.h from the half rows or the palette tables) and trilerp. The gradient is the trilinear
// interpolation, by the same trilerp, of the central differences of the node values at the 8 corners: 48 node values a point,
// of which a mesh vertex (on a lattice edge) weights 12 with anything but zero. No LDS, no atomics; a point writes only its own
// rows of the outputs.
#include "grid_fetch_device.h"

namespace nerf {
namespace {

// the node value of the extraction (McGridVolume::at of mesh_kernels.hip): 0 at an empty or masked-out node
__device__ __forceinline__ float node_value(const GridDev& g, const uint8_t* mask, int64_t p) {
    const int32_t l = g.links[p];
    if (l < 0 || (int64_t)l >= g.capacity) return 0.0f;
    if (mask && !mask[p]) return 0.0f;
    return g.density[l];
}

// G(q)_b = h_b (v(q + e_b) - v(q - e_b)); a neighbour outside the lattice is q itself, h_b = 1 at such a border node, else 0.5
__device__ __forceinline__ void node_gradient(const GridDev& g, const uint8_t* mask, const int q[3], float G[3]) {
    const int64_t stride[3] = {(int64_t)g.size[1] * g.size[2], (int64_t)g.size[2], 1};
    const int64_t p = q[0] * stride[0] + q[1] * stride[1] + q[2];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const bool lo = q[b] > 0, hi = q[b] + 1 < g.size[b];
        const float vp = node_value(g, mask, hi ? p + stride[b] : p);
        const float vm = node_value(g, mask, lo ? p - stride[b] : p);
        G[b] = mul(lo && hi ? 0.5f : 1.0f, sub(vp, vm));
    }
}

// coefficient k of channel c of a row, per kind of colour table
struct RowFloat {
    const float* base;
    int row;
    __device__ __forceinline__ RowFloat(const GridDev& g, const GridPalette&, const GridMeshAttr&, int B, int c, int k)
        : base(g.sh + c * B + k), row(3 * B) {}
    __device__ __forceinline__ float at(int link) const { return base[(int64_t)link * row]; }
};
struct RowHalf {
    const uint16_t* base;
    int row;
    __device__ __forceinline__ RowHalf(const GridDev& g, const GridPalette&, const GridMeshAttr& a, int, int c, int k)
        : base(g.sh_half + c * a.half_channel + k), row(a.half_row) {}
    __device__ __forceinline__ float at(int link) const { return widen(base[(int64_t)link * row]); }
};
struct RowPalette {
    PaletteLane f;
    __device__ __forceinline__ RowPalette(const GridDev&, const GridPalette& p, const GridMeshAttr&, int B, int c, int k)
        : f(p, B, c, k) {}
    __device__ __forceinline__ float at(int link) const { return f.at(link); }
};

template <class Row>
__global__ __launch_bounds__(kGridThreads) void grid_mesh_attributes_kernel(GridDev g, GridPalette pal, GridMeshAttr a) {
    const int64_t idx = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (idx >= a.n) return;
    const float x[3] = {a.points[idx * 3 + 0], a.points[idx * 3 + 1], a.points[idx * 3 + 2]};
    int l[3];
    float wa[3], wb[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        cell_of(x[i], g.size[i], l[i], wb[i]);
        wa[i] = sub(1.0f, wb[i]);
    }
    const int base = (l[0] * g.size[1] + l[1]) * g.size[2] + l[2];      // point_cell's

    float nrm[3] = {0.0f, 0.0f, 0.0f};
    if (a.normals || a.color_mode == NERF_GRID_MESH_COLOR_SH) {
        float gv[3][8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int q[3] = {l[0] + ((c >> 2) & 1), l[1] + ((c >> 1) & 1), l[2] + (c & 1)};
            float G[3];
            node_gradient(g, a.mask, q, G);
            gv[0][c] = G[0];
            gv[1][c] = G[1];
            gv[2][c] = G[2];
        }
        // world gradient: d / d world_b = scaling_b d / d grid_b, scaling_b = reso_b / (2 radius_b)
        float gw[3];
#pragma unroll
        for (int b = 0; b < 3; ++b) gw[b] = mul(trilerp(gv[b], wa, wb), g.scaling[b]);
        // scaled by its largest component first: the length neither overflows nor vanishes where the gradient does not
        const float m = fmaxf(fmaxf(fabsf(gw[0]), fabsf(gw[1])), fabsf(gw[2]));
        if (m > 0.0f && isfinite(m)) {
            const float s[3] = {gw[0] / m, gw[1] / m, gw[2] / m};
            const float len = sqrtf(add(add(mul(s[0], s[0]), mul(s[1], s[1])), mul(s[2], s[2])));
            if (len > 0.0f && isfinite(len)) {
#pragma unroll
                for (int b = 0; b < 3; ++b) nrm[b] = -(s[b] / len);
            }
        }
        if (a.normals) {
#pragma unroll
            for (int b = 0; b < 3; ++b) a.normals[idx * 3 + b] = nrm[b];
        }
    }
    if (a.color_mode == NERF_GRID_MESH_COLOR_NONE) return;

    float d[3] = {a.view[0], a.view[1], a.view[2]};
    bool dc = a.color_mode == NERF_GRID_MESH_COLOR_DC;
    if (a.color_mode == NERF_GRID_MESH_COLOR_SH) {
        // the ray that meets the surface head-on; without a normal there is no such ray
        dc = nrm[0] == 0.0f && nrm[1] == 0.0f && nrm[2] == 0.0f;
#pragma unroll
        for (int b = 0; b < 3; ++b) d[b] = -nrm[b];
    }
    int lk[8];
    load_links(g, base, lk);
    const int B = g.basis_dim, nk = dc ? 1 : B;
    for (int c = 0; c < 3; ++c) {
        float acc = 0.0f;
        for (int k = 0; k < nk; ++k) {
            const Row row(g, pal, a, B, c, k);
            float cv[8];
#pragma unroll
            for (int v = 0; v < 8; ++v) cv[v] = lk[v] >= 0 ? row.at(lk[v]) : 0.0f;
            const float term = mul(trilerp(cv, wa, wb), sh_basis(k, d[0], d[1], d[2]));
            acc = k == 0 ? term : add(acc, term);
        }
        a.colors[idx * 3 + c] = fminf(fmaxf(add(0.5f, acc), 0.0f), 1.0f);
    }
}

}  // namespace

hipError_t launch_grid_mesh_attributes(const GridDev& g, const GridPalette& p, bool half, bool palette, const GridMeshAttr& a,
                                       hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    GridMeshAttr b = a;
    b.half_channel = grid_half_channel_halfs(g.basis_dim);
    b.half_row = grid_half_row_halfs(g.basis_dim);
    if (palette)
        grid_mesh_attributes_kernel<RowPalette><<<blocks_for(a.n), kGridThreads, 0, s>>>(g, p, b);
    else if (half)
        grid_mesh_attributes_kernel<RowHalf><<<blocks_for(a.n), kGridThreads, 0, s>>>(g, p, b);
    else
        grid_mesh_attributes_kernel<RowFloat><<<blocks_for(a.n), kGridThreads, 0, s>>>(g, p, b);
    return hipGetLastError();
}

}  // namespace nerf
