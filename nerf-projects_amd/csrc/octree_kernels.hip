// PlenOctree: the cell-to-cell march of an N3Tree and the build of such a tree from a sparse voxel grid.
// Semantics: include/nerf_mi355x.h, "PlenOctree". Design and measurements: DESIGN.md section 7s, profiles/octree.md.
//
// Render mapping: one lane per ray. A sample is a chain of dependent loads - up to max_depth + 1 `child` words, then the
// leaf's sigma - and only a sample above sigma_thresh touches the 3 B colours of its row, which the lane reads itself in a loop
// over the coefficients. The SH basis depends on the ray alone and is made once, before the march, into B registers: every
// index into it is a compile-time constant after unrolling (dispatch_octree_basis), so nothing lives in scratch. No LDS, no
// shuffles in the kept mapping: every result depends on its own ray only, and two runs give the same bits.
// The image form makes its rays in the launch, an 8 x 8 tile of pixels per wavefront (grid_depth_kernels.hip has the reason);
// the ray form maps consecutive rays.
// nerf_octree_accelerate's table starts a descent below the root (octree_descend<true>): a compile-time variant of the same
// kernel, the same bits. The device functions of the march live in octree_device.h, shared with octree_grad_kernels.hip.
#include "compact_device.h"
#include "grid_device.h"
#include "octree_device.h"
#include "octree_internal.h"

namespace nerf {
namespace {

template <int B, bool IMAGE, bool ACCEL>
__global__ __launch_bounds__(kGridThreads) void octree_render_kernel(OctreeDev t, OctreeRenderOpt opt, OctreeRender r) {
    const int64_t tid = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    int64_t ray;
    float ow[3], dw[3];
    if (IMAGE) {
        ray = tile_pixel(r.cam, tid);
        if (ray < 0) return;
        camera_ray(r.cam, ray, ow, dw);
    } else {
        ray = tid;
        if (ray >= r.n_rays) return;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            ow[i] = r.origins[ray * 3 + i];
            dw[i] = r.dirs[ray * 3 + i];
        }
    }
    OctreeRay rs;
    octree_setup(t, ow, dw, rs);
    float rgb[3] = {0.0f, 0.0f, 0.0f};
    int steps = 0;
    bool done = false;      // the ray ended at stop_thresh: no background term
    if (!rs.ok) {
        rgb[0] = rgb[1] = rgb[2] = __builtin_nanf("");
        done = true;
    }
    float T = 1.0f;
    if (rs.ok && !(rs.tmax < 0.0f) && !(rs.tmin > rs.tmax)) {
        float basis[B];
        octree_sh_basis<B>(dw[0], dw[1], dw[2], basis);
        const float hi = sub(1.0f, 1e-6f);
        float tt = rs.tmin;
        while (tt < rs.tmax) {
            if (steps >= kOctreeMaxIters) {
                if (r.capped) atomicAdd(r.capped, 1ull);
                break;
            }
            ++steps;
            float p[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) p[i] = fminf(fmaxf(add(rs.o[i], mul(tt, rs.d[i])), 0.0f), hi);
            float inv_cube;
            const int64_t cell = octree_descend<ACCEL>(t, p, inv_cube);
            float a, b;
            unit_cube(p, rs.inv, a, b);
            // (b - a) / cube: cube is a power of two, so the product with its reciprocal is that quotient, bit for bit
            const float delta = add(mul(sub(b, a), inv_cube), opt.step_size);
            const float* row = t.data + cell * t.data_dim;
            const float sigma = row[3 * B];
            if (sigma > opt.sigma_thresh) {
                const float att = expf(mul(mul(-delta, rs.delta_scale), sigma));
                const float weight = mul(T, sub(1.0f, att));
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float s = mul(basis[0], row[c * B]);
#pragma unroll
                    for (int i = 1; i < B; ++i) s = add(s, mul(basis[i], row[c * B + i]));
                    rgb[c] = add(rgb[c], mul(weight, octree_act(t.act, s)));
                }
                T = mul(T, att);
                if (T <= opt.stop_thresh) {
                    const float scale = __fdiv_rn(1.0f, sub(1.0f, T));
#pragma unroll
                    for (int c = 0; c < 3; ++c) rgb[c] = mul(rgb[c], scale);
                    done = true;
                    break;
                }
            }
            const float tn = add(tt, delta);
            if (!(tn > tt)) break;
            tt = tn;
        }
    }
    if (!done) {
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[c] = add(rgb[c], mul(T, opt.background_brightness));
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) r.rgb[ray * 3 + c] = rgb[c];
    if (r.steps) r.steps[ray] = steps;
}

// one thread per table cell: the integer twin of the descent, the cell's bits from the top down
__global__ __launch_bounds__(kGridThreads) void octree_table_kernel(OctreeDev t, int levels, int2* table) {
    const int64_t i = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (i >= (int64_t)1 << (3 * levels)) return;
    const int mask = (1 << levels) - 1;
    const int x = (int)(i >> (2 * levels)), y = (int)(i >> levels) & mask, z = (int)i & mask;
    int64_t node = 0, cell = 0;
    int depth = 0;
    while (depth < levels) {
        const int bit = levels - 1 - depth;
        cell = node * 8 + (((x >> bit) & 1) * 4 + ((y >> bit) & 1) * 2 + ((z >> bit) & 1));
        ++depth;
        const int32_t skip = t.child[cell];
        if (skip == 0) break;
        node += skip;
    }
    table[i] = make_int2((int)cell, depth);
}

__global__ __launch_bounds__(kGridThreads) void octree_check_child_kernel(const int32_t* child, int64_t n_nodes, int* out) {
    const int64_t i = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (i >= n_nodes * 8) return;
    const int32_t v = child[i];
    if (v < 0 || (v > 0 && i / 8 + v >= n_nodes)) *out = 1;      // (every writer stores the same value)
}

// ---- build from a grid ------------------------------------------------------------------------------------------------------
// cell (x, y, z) of a level with `side` cells per axis, C order
__device__ __forceinline__ int64_t cell_index(int x, int y, int z, int side) { return ((int64_t)x * side + y) * side + z; }

// occ of a level from the level below it (FROM_LINKS: from the grid's links, a kept node is links >= 0): the OR of 8
template <bool FROM_LINKS>
__global__ __launch_bounds__(kGridThreads) void octree_occupancy_kernel(const void* below, int side, uint8_t* occ) {
    const int64_t i = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (i >= (int64_t)side * side * side) return;
    const int z = (int)(i % side), y = (int)((i / side) % side), x = (int)(i / ((int64_t)side * side));
    bool any = false;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int64_t j = cell_index(2 * x + (c >> 2), 2 * y + ((c >> 1) & 1), 2 * z + (c & 1), 2 * side);
        any = any || (FROM_LINKS ? ((const int32_t*)below)[j] >= 0 : ((const uint8_t*)below)[j] != 0);
    }
    occ[i] = any ? 1 : 0;
}

// base[0] = 0 (the root), base[l] = 1 + the nodes of depths 1 .. l - 1, base[levels] = the node count
__global__ void octree_bases_kernel(const int32_t* counts, int levels, int32_t* base) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int32_t run = 1;
    base[0] = 0;
    for (int l = 1; l < levels; ++l) {
        base[l] = run;
        run += counts[l];
    }
    base[levels] = run;
}

// One thread per cell of level l + 1 (side2 = 2^(l + 1) cells per axis): the cell (u, v, w) of the node of depth l above it,
// if that node exists. It writes the cell's child entry and data row, and, in the node's first cell, parent_depth.
__global__ __launch_bounds__(kGridThreads) void octree_fill_kernel(OctreeBuild b, int l) {
    const int side2 = 2 << l;
    const int64_t i = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (i >= (int64_t)side2 * side2 * side2) return;
    const int z = (int)(i % side2), y = (int)((i / side2) % side2), x = (int)(i / ((int64_t)side2 * side2));
    const int32_t* base = (const int32_t*)(b.ws + b.lay.base);
    int64_t node = 0;
    if (l > 0) {
        const int32_t rk = ((const int32_t*)(b.ws + b.lay.rank[l]))[cell_index(x >> 1, y >> 1, z >> 1, side2 >> 1)];
        if (rk < 0) return;
        node = (int64_t)base[l] + rk;
    }
    if (node >= b.n_nodes) return;      // (the grid changed between the two calls: nothing is written outside the arrays)
    const int uvw = (x & 1) * 4 + (y & 1) * 2 + (z & 1);
    const int64_t cell = node * 8 + uvw;
    const int D = 3 * b.basis_dim + 1;
    float* row = b.data + cell * D;
    int32_t child = 0;
    int32_t link = -1;
    if (l + 1 < b.levels) {
        const int32_t rk = ((const int32_t*)(b.ws + b.lay.rank[l + 1]))[i];
        if (rk >= 0) child = (int32_t)((int64_t)base[l + 1] + rk - node);
    } else {
        link = b.links[i];
    }
    b.child[cell] = child;
    if (link >= 0) {
        for (int j = 0; j < D - 1; ++j) row[j] = b.sh[(int64_t)link * (D - 1) + j];
        row[D - 1] = b.density[link];
    } else {
        for (int j = 0; j < D; ++j) row[j] = 0.0f;
    }
    if (uvw == 0) {
        int64_t parent_cell = 0;
        if (l > 0) {
            const int px = x >> 1, py = y >> 1, pz = z >> 1;      // this node's own cell, of level l
            int64_t parent = 0;
            if (l > 1) parent = (int64_t)base[l - 1] + ((const int32_t*)(b.ws + b.lay.rank[l - 1]))[cell_index(px >> 1, py >> 1, pz >> 1, side2 >> 2)];
            parent_cell = parent * 8 + (px & 1) * 4 + (py & 1) * 2 + (pz & 1);
        }
        b.parent_depth[node * 2] = (int32_t)parent_cell;
        b.parent_depth[node * 2 + 1] = l;
    }
}

}  // namespace

void octree_build_layout(int levels, OctreeBuildLayout* lay) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t off = 0;
    lay->levels = levels;
    size_t largest = 1;
    for (int l = 0; l < 11; ++l) lay->occ[l] = lay->rank[l] = 0;
    for (int l = 1; l < levels; ++l) {
        const size_t cells = (size_t)1 << (3 * l);
        lay->occ[l] = off;
        off += up(cells);
        lay->rank[l] = off;
        off += up(cells * sizeof(int32_t));
        largest = cells;
    }
    lay->counts = off;
    off += up(16 * sizeof(int32_t));
    lay->base = off;
    off += up(16 * sizeof(int32_t));
    lay->block_offsets = off;
    off += up((size_t)compact_blocks((int64_t)largest) * sizeof(int32_t));
    lay->total = off;
}

hipError_t launch_octree_check_child(const int32_t* child, int64_t n_nodes, int* out, hipStream_t s) {
    hipError_t e = hipMemsetAsync(out, 0, sizeof(int), s);
    if (e != hipSuccess) return e;
    octree_check_child_kernel<<<blocks_for(n_nodes * 8), kGridThreads, 0, s>>>(child, n_nodes, out);
    return hipGetLastError();
}

hipError_t launch_octree_render(const OctreeDev& t, const OctreeRenderOpt& o, const OctreeRender& r, hipStream_t s) {
    if (r.n_rays <= 0) return hipSuccess;
    return dispatch_octree_basis(t.basis_dim, [&](auto bd) {
        constexpr int B = decltype(bd)::value;
        const bool image = r.origins == nullptr;
        const unsigned blocks = blocks_for(image ? image_threads(r.cam) : r.n_rays);
        if (t.table) {
            if (image) octree_render_kernel<B, true, true><<<blocks, kGridThreads, 0, s>>>(t, o, r);
            else octree_render_kernel<B, false, true><<<blocks, kGridThreads, 0, s>>>(t, o, r);
        } else {
            if (image) octree_render_kernel<B, true, false><<<blocks, kGridThreads, 0, s>>>(t, o, r);
            else octree_render_kernel<B, false, false><<<blocks, kGridThreads, 0, s>>>(t, o, r);
        }
        return hipGetLastError();
    });
}

hipError_t launch_octree_table(const OctreeDev& t, int levels, int2* table, hipStream_t s) {
    octree_table_kernel<<<blocks_for((int64_t)1 << (3 * levels)), kGridThreads, 0, s>>>(t, levels, table);
    return hipGetLastError();
}

hipError_t launch_octree_plan(const OctreeBuild& b, hipStream_t s) {
    const int L = b.levels;
    int32_t* counts = (int32_t*)(b.ws + b.lay.counts);
    hipError_t e = hipMemsetAsync(counts, 0, 16 * sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    for (int l = L - 1; l >= 1; --l) {
        const int side = 1 << l;
        const int64_t cells = (int64_t)side * side * side;
        uint8_t* occ = (uint8_t*)(b.ws + b.lay.occ[l]);
        if (l == L - 1)
            octree_occupancy_kernel<true><<<blocks_for(cells), kGridThreads, 0, s>>>(b.links, side, occ);
        else
            octree_occupancy_kernel<false><<<blocks_for(cells), kGridThreads, 0, s>>>(b.ws + b.lay.occ[l + 1], side, occ);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    for (int l = 1; l < L; ++l) {
        const int64_t cells = (int64_t)1 << (3 * l);
        e = launch_grid_compact((const uint8_t*)(b.ws + b.lay.occ[l]), cells, (int32_t*)(b.ws + b.lay.block_offsets),
                                (int32_t*)(b.ws + b.lay.rank[l]), counts + l, s);
        if (e != hipSuccess) return e;
    }
    octree_bases_kernel<<<1, 64, 0, s>>>(counts, L, (int32_t*)(b.ws + b.lay.base));
    return hipGetLastError();
}

hipError_t launch_octree_fill(const OctreeBuild& b, hipStream_t s) {
    for (int l = 0; l < b.levels; ++l) {
        const int64_t cells = (int64_t)1 << (3 * (l + 1));
        octree_fill_kernel<<<blocks_for(cells), kGridThreads, 0, s>>>(b, l);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace nerf
