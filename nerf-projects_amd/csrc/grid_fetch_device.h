// Sparse voxel grid: how one SH coefficient of one node's row is read from the colour tables that are not fp32 - the packed
// half rows (grid_half_kernels.hip) and the palette tables (grid_palette_kernels.hip). Shared by those samplers and by the
// mesh attribute kernel (grid_mesh_kernels.hip), so that all of them see the same value, bit for bit.
#pragma once
#include "grid_device.h"

namespace nerf {
namespace {

__device__ __forceinline__ float widen(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }

// what lane (c, k) reads of a node: set up once per lane, before the march
struct PaletteLane {
    const uint16_t* map;       // &map[k - retain], or nullptr: a retained function
    const uint16_t* value;     // &colors[k - retain][0][c], or &retained[0][k][c]
    int stride;                // halfs from a node's row to the next, of map / of retained

    __device__ __forceinline__ PaletteLane(const GridPalette& p, int B, int c, int k) {
        if (k < p.retain) {
            map = nullptr;
            value = p.retained + k * 3 + c;
            stride = 3 * p.retain;
        } else {
            const int q = k - p.retain;
            map = p.map + q;
            value = p.colors + (int64_t)q * p.entries * 3 + c;
            stride = B - p.retain;
        }
    }
    __device__ __forceinline__ float at(int link) const {
        if (map) return widen(value[(int)map[(int64_t)link * stride] * 3]);
        return widen(value[(int64_t)link * stride]);
    }
};

}  // namespace
}  // namespace nerf
