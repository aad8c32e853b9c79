// Sparse voxel grid (Plenoxels) resampling: the stages of svox2's SparseGrid.resample as kernels - the density of the old
// grid on a new lattice, the per-camera maximum-weight render over that dense volume, threshold and dilation of the keep mask,
// the compaction of the mask into links, and the gather of the new tables. Semantics: include/nerf_mi355x.h, "Sparse voxel
// grid: resampling". Design and measurements: DESIGN.md section 7e.
//
// Everything that interpolates goes through grid_device.h (cell_of, load_links, trilerp, the rounded add / mul / sub): a
// resampled value is the value grid_sample_kernel gives at the same point, bit for bit. Node counts reach 1024^3 = 2^30 and
// rows * columns passes 2^31 at 512^3 * 27, so every flat index is int64_t. No scratch, no inline assembly; LDS only in the
// compaction (compact_device.h: 16 ballots per workgroup and the one-workgroup scan); the only atomic is the weight render's
// integer maximum.
#include "compact_device.h"
#include "grid_device.h"

namespace nerf {
namespace {

// ---- lattice density: one thread per node of the new lattice, z fastest ------------------------------------------------
__global__ __launch_bounds__(kGridThreads) void grid_lattice_density_kernel(GridDev g, GridLattice a) {
    const int64_t n = (int64_t)a.size[0] * a.size[1] * a.size[2];
    const int64_t idx = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (idx >= n) return;
    int ix, iy, iz;
    node_to_xyz(idx, a.size, ix, iy, iz);
    const float p[3] = {a.axis[0][ix], a.axis[1][iy], a.axis[2][iz]};
    float wa[3], wb[3];
    int lk[8];
    load_links(g, point_cell(g, p, wa, wb), lk);
    a.density[idx] = sample_sigma(g, lk, wa, wb);
}

// ---- weight render: one thread per pixel (svox2 grid_weight_render) -----------------------------------------------------
// weight >= 0, so the order of the floats is the order of their bits: one integer maximum, whose result does not depend on
// the order of arrival. The 8 entries are first read with plain global loads issued together (one wait for all of them), and
// an entry already >= weight needs no atomic; a stale (smaller) value read costs one atomic that changes nothing, never a
// missed update, because entries only grow. (DESIGN.md 7e has the A/B against the form without the loads.)
__device__ __forceinline__ void raise_corners(float* p, int64_t s0, int64_t s1, float weight) {
    float* q[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) q[c] = p + ((c >> 2) & 1) * s0 + ((c >> 1) & 1) * s1 + (c & 1);
    float cur[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) cur[c] = *q[c];
#pragma unroll
    for (int c = 0; c < 8; ++c)
        if (!(cur[c] >= weight)) atomicMax(reinterpret_cast<unsigned int*>(q[c]), __float_as_uint(weight));
}

__global__ __launch_bounds__(kGridThreads) void grid_weight_render_kernel(GridWeight a) {
    const int64_t pix = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (pix >= (int64_t)a.cam.width * a.cam.height) return;
    float o[3], d[3];
    camera_ray(a.cam, pix, o, d);      // the renderer's own ray (grid_device.h)
    // the ray set-up of the renderer (grid_device.h setup_ray) on this lattice, with t starting at 0 and tmax at 2e3
    const float dn = sqrtf(add(add(mul(d[0], d[0]), mul(d[1], d[1])), mul(d[2], d[2])));
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        o[i] = add(a.offset[i], mul(o[i], a.scaling[i]));
        d[i] = mul(d[i] / dn, a.scaling[i]);
    }
    const float delta_scale = 1.0f / sqrtf(add(add(mul(d[0], d[0]), mul(d[1], d[1])), mul(d[2], d[2])));
    const float world_step = mul(delta_scale, a.step_size);
    float t = 0.0f, tmax = 2e3f;
    bool ok = dn > 0.0f && isfinite(dn) && isfinite(delta_scale);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        d[i] = mul(d[i], delta_scale);
        const float inv = 1.0f / d[i];
        const float t1 = mul(sub(-0.5f, o[i]), inv);
        const float t2 = mul(sub((float)a.size[i] - 0.5f, o[i]), inv);
        if (d[i] != 0.0f) {
            t = fmaxf(t, fminf(t1, t2));
            tmax = fminf(tmax, fmaxf(t1, t2));
        }
        ok = ok && isfinite(o[i]) && isfinite(d[i]);
    }
    if (!ok || !isfinite(t) || !(t <= tmax)) return;      // a miss, or a set-up that is not finite: nothing is marched
    const int64_t s0 = (int64_t)a.size[1] * a.size[2], s1 = a.size[2];
    const float neg_world_step = -world_step;
    float log_t = 0.0f;
    while (t <= tmax) {
        const float t_next = add(t, a.step_size);
        if (!(t_next > t)) break;      // (cannot happen below tmax = 2e3 with step_size >= 1e-3; the march ends regardless)
        int l[3];
        float wa[3], wb[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            cell_of(add(o[i], mul(t, d[i])), a.size[i], l[i], wb[i]);
            wa[i] = sub(1.0f, wb[i]);
        }
        const int64_t base = ((int64_t)l[0] * a.size[1] + l[1]) * a.size[2] + l[2];
        float cv[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) cv[c] = a.density[base + ((c >> 2) & 1) * s0 + ((c >> 1) & 1) * s1 + (c & 1)];
        const float sigma = trilerp(cv, wa, wb);
        if (sigma > 1e-8f) {
            const float log_att = mul(neg_world_step, sigma);
            const float weight = mul(expf(log_t), sub(1.0f, expf(log_att)));
            log_t = add(log_t, log_att);
            raise_corners(a.max_weight + base, s0, s1, weight);
            if (expf(log_t) < a.stop_thresh) break;
        }
        t = t_next;
    }
}

// ---- keep mask ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kGridThreads) void grid_threshold_kernel(const float* __restrict__ volume, int64_t n, float threshold,
                                                                       uint8_t* __restrict__ mask) {
    const int64_t idx = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (idx >= n) return;
    mask[idx] = volume[idx] >= threshold ? 1 : 0;      // (NaN is not kept)
}

// one step of the 27-neighbourhood OR, indices clamped at the faces (svox2 dilate_kernel)
__global__ __launch_bounds__(kGridThreads) void grid_dilate_kernel(const uint8_t* __restrict__ in, int sx, int sy, int sz,
                                                                    uint8_t* __restrict__ out) {
    const int64_t n = (int64_t)sx * sy * sz;
    const int64_t idx = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (idx >= n) return;
    const int32_t size[3] = {sx, sy, sz};
    int x, y, z;
    node_to_xyz(idx, size, x, y, z);
    const int xs[3] = {max(x - 1, 0), x, min(x + 1, sx - 1)};
    const int ys[3] = {max(y - 1, 0), y, min(y + 1, sy - 1)};
    const int zs[3] = {max(z - 1, 0), z, min(z + 1, sz - 1)};
    uint8_t v = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const uint8_t* row = in + ((int64_t)xs[a] * sy + ys[b]) * sz;
            v |= row[zs[0]] | row[zs[1]] | row[zs[2]];
        }
    out[idx] = v ? 1 : 0;
}

// ---- compaction: mask -> links (compact_device.h: count per workgroup, scan, rank) ------------------------------------------
__global__ __launch_bounds__(kGridThreads) void grid_compact_count_kernel(const uint8_t* __restrict__ mask, int64_t n,
                                                                           int32_t* __restrict__ block_offsets) {
    int kept = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t node = compact_item(r);
        kept += __popcll(__ballot(node < n && mask[node] != 0));
    }
    compact_store_count(kept, block_offsets);
}

// one workgroup turns the per-workgroup counts into exclusive offsets (in place) and stores the total
__global__ __launch_bounds__(1024) void grid_compact_scan_kernel(int32_t* counts, int64_t n, int32_t* total) {
    const int v = compact_scan(counts, n);
    if (threadIdx.x == 1023) *total = v;
}

__global__ __launch_bounds__(kGridThreads) void grid_compact_links_kernel(const uint8_t* __restrict__ mask, int64_t n,
                                                                           const int32_t* __restrict__ block_offsets,
                                                                           int32_t* __restrict__ links) {
    bool keep[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t node = compact_item(r);
        keep[r] = node < n && mask[node] != 0;
    }
    const CompactRanks ranks = compact_ranks(keep, block_offsets);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t node = compact_item(r);
        if (node < n) links[node] = keep[r] ? ranks.rank(r) : -1;
    }
}

// ---- gather ---------------------------------------------------------------------------------------------------------------
// node_of_row[links[node]] = node: the inverse of the compaction, so that the gather can run over rows
__global__ __launch_bounds__(kGridThreads) void grid_row_nodes_kernel(const int32_t* __restrict__ links, int64_t n, int64_t rows,
                                                                       int32_t* __restrict__ node_of_row) {
    const int64_t idx = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    if (idx >= n) return;
    const int32_t row = links[idx];
    if (row >= 0 && (int64_t)row < rows) node_of_row[row] = (int32_t)idx;
}

// one thread per (row, SH column): consecutive lanes write consecutive floats of sh_data; the lane of column 0 also copies
// the row's density from the lattice volume (the value the threshold saw)
__global__ __launch_bounds__(kGridThreads) void grid_gather_kernel(GridDev g, GridGather a) {
    const int cols = 3 * g.basis_dim;
    const int64_t tid = (int64_t)blockIdx.x * kGridThreads + threadIdx.x;
    const int64_t row = tid / cols;
    const int j = (int)(tid % cols);
    if (row >= a.rows) return;
    const int64_t node = a.node_of_row[row];
    if (node < 0 || node >= (int64_t)a.size[0] * a.size[1] * a.size[2]) return;      // (links that are no compaction: nothing is read)
    int ix, iy, iz;
    node_to_xyz(node, a.size, ix, iy, iz);
    const float p[3] = {a.axis[0][ix], a.axis[1][iy], a.axis[2][iz]};
    float wa[3], wb[3];
    int lk[8];
    load_links(g, point_cell(g, p, wa, wb), lk);
    float cv[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) cv[c] = lk[c] >= 0 ? g.sh[(int64_t)lk[c] * cols + j] : 0.0f;
    a.sh_data[row * cols + j] = trilerp(cv, wa, wb);
    if (j == 0) a.density_data[row] = a.lattice_density[node];
}

}  // namespace

hipError_t launch_grid_lattice_density(const GridDev& g, const GridLattice& a, hipStream_t s) {
    const int64_t n = (int64_t)a.size[0] * a.size[1] * a.size[2];
    grid_lattice_density_kernel<<<blocks_for(n), kGridThreads, 0, s>>>(g, a);
    return hipGetLastError();
}

hipError_t launch_grid_weight_render(const GridWeight& a, hipStream_t s) {
    grid_weight_render_kernel<<<blocks_for((int64_t)a.cam.width * a.cam.height), kGridThreads, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_grid_threshold(const float* volume, int64_t n, float threshold, uint8_t* mask, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    grid_threshold_kernel<<<blocks_for(n), kGridThreads, 0, s>>>(volume, n, threshold, mask);
    return hipGetLastError();
}

hipError_t launch_grid_dilate(const uint8_t* in, const int32_t size[3], uint8_t* out, hipStream_t s) {
    const int64_t n = (int64_t)size[0] * size[1] * size[2];
    grid_dilate_kernel<<<blocks_for(n), kGridThreads, 0, s>>>(in, size[0], size[1], size[2], out);
    return hipGetLastError();
}

hipError_t launch_grid_compact(const uint8_t* mask, int64_t n, int32_t* block_offsets, int32_t* links, int32_t* count,
                               hipStream_t s) {
    const int64_t nb = compact_blocks(n);
    grid_compact_count_kernel<<<(unsigned)nb, kGridThreads, 0, s>>>(mask, n, block_offsets);
    grid_compact_scan_kernel<<<1, 1024, 0, s>>>(block_offsets, nb, count);
    grid_compact_links_kernel<<<(unsigned)nb, kGridThreads, 0, s>>>(mask, n, block_offsets, links);
    return hipGetLastError();
}

hipError_t launch_grid_gather(const GridDev& g, const GridGather& a, hipStream_t s) {
    if (a.rows <= 0) return hipSuccess;
    const int64_t n = (int64_t)a.size[0] * a.size[1] * a.size[2];
    // a row no link names keeps node 0: whatever `links` holds, the gather reads inside the lattice
    hipError_t e = hipMemsetAsync(a.node_of_row, 0, (size_t)a.rows * sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    grid_row_nodes_kernel<<<blocks_for(n), kGridThreads, 0, s>>>(a.links, n, a.rows, a.node_of_row);
    grid_gather_kernel<<<blocks_for(a.rows * 3 * g.basis_dim), kGridThreads, 0, s>>>(g, a);
    return hipGetLastError();
}

}  // namespace nerf
