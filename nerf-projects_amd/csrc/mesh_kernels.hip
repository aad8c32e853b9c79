// Marching cubes on a device volume (nerf_marching_cubes, include/nerf_mi355x.h): the mesh step of gen_mesh.py:124
// (mcubes.marching_cubes) on the GPU, deterministic and without atomics on the output path.
//
// Four passes over the volume [X, Y, Z] (fp32, C order) and one scan:
//   mc_edge_count_kernel     per lattice point: which of its three forward edges cross the isovalue (3 bits), and the point's
//                            exclusive prefix of crossing edges inside its tile of kMcTile points; per tile: the count
//   mc_cell_count_kernel     per cell: the case index and the triangle count of that case; per tile of kMcTile cells: the count
//   mc_scan_kernel           the two tile counts -> int64 exclusive offsets and totals (one workgroup per array)
//   mc_vertex_kernel         every crossing edge writes its vertex at rank(edge key 3 * linear_index + axis)
//   mc_triangle_kernel       every cell writes its triangles at (tile offset + prefix inside the tile), vertex ids looked up
//                            through the per-point record of the first pass
// The per-point record is 16 bits: the prefix (< 3 * kMcTile = 6144, 13 bits) << 3 | the crossing mask. The triangle table
// is generated once on the host (build_tri_table) and copied to __constant__ memory.
//
// The kernels are templates over where a node's value comes from (McVolume, McGridVolume below): nerf_grid_marching_cubes
// (include/nerf_mi355x.h, "Sparse voxel grid: surface meshes") runs the same passes on a sparse voxel grid's links and
// density table, and so returns what nerf_marching_cubes returns on the densified volume, bit for bit and in order.
#include <cstring>
#include <mutex>

#include "nerf_internal.h"

namespace nerf {

namespace {

constexpr int kMcThreads = 256;
constexpr int kMcPer = 8;                         // consecutive items per thread
constexpr int kMcTile = kMcThreads * kMcPer;      // items (points or cells) per workgroup

// Cube corner v = 4 di + 2 dj + dk: the lattice point (i + di, j + dj, k + dk) of cell (i, j, k). Edge e runs from corner
// kEdgeCorner[e] along axis kEdgeAxis[e] (axis 0, 1, 2 = x, y, z): the x edges first, then y, then z.
__constant__ int8_t c_edge_corner[12] = {0, 1, 2, 3, 0, 1, 4, 5, 0, 2, 4, 6};
__constant__ int8_t c_edge_axis[12] = {0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2};
__constant__ int8_t c_tri[256][16];               // up to 5 triangles as edge triples, -1 terminated
__constant__ int8_t c_ntri[256];

__device__ __forceinline__ bool mc_inside(float v, float iso) { return v >= iso; }      // NaN is outside

// Where the node values come from. A source has X, Y, Z, iso, at(p) = the value of lattice point p (C order) and
// load_run(p0, P, v) = the kMcPer values from p0 on (0 past the end). Every kernel below is written once over a source: the
// passes, the records, the order and the arithmetic of a vertex are the same for all of them.
//
// a dense fp32 volume (nerf_marching_cubes)
struct McVolume {
    const float* v;
    uint32_t X, Y, Z;
    float iso;
    int vec;            // 16-byte aligned: a thread's own 8 values come in two 16-byte loads

    __device__ __forceinline__ float at(uint32_t p) const { return v[p]; }
    // the thread's kMcPer values starting at lattice point p0 (vector loads when they all exist and the volume is aligned)
    __device__ __forceinline__ void load_run(uint32_t p0, uint32_t P, float (&out)[kMcPer]) const {
        if (vec && p0 + kMcPer <= P) {
            const float4 a = *(const float4*)(v + p0);
            const float4 b = *(const float4*)(v + p0 + 4);
            out[0] = a.x; out[1] = a.y; out[2] = a.z; out[3] = a.w;
            out[4] = b.x; out[5] = b.y; out[6] = b.z; out[7] = b.w;
        } else {
#pragma unroll
            for (int q = 0; q < kMcPer; ++q) out[q] = p0 + q < P ? v[p0 + q] : 0.0f;
        }
    }
};

// a sparse voxel grid (nerf_grid_marching_cubes): the density of the node's row where its link is kept and its mask byte is
// not 0, else 0. Only `links` is streamed; a density is gathered where a link is kept, and no volume is written anywhere.
struct McGridVolume {
    const int32_t* links;
    const float* density;
    const uint8_t* mask;      // [X, Y, Z] or nullptr
    int64_t capacity;
    uint32_t X, Y, Z;
    float iso;
    int vec;            // links 16-byte aligned

    __device__ __forceinline__ float value(int32_t link, uint32_t p) const {
        if (link < 0 || (int64_t)link >= capacity) return 0.0f;
        if (mask && !mask[p]) return 0.0f;
        return density[link];
    }
    __device__ __forceinline__ float at(uint32_t p) const { return value(links[p], p); }
    __device__ __forceinline__ void load_run(uint32_t p0, uint32_t P, float (&out)[kMcPer]) const {
        if (vec && p0 + kMcPer <= P) {
            const int4 a = *(const int4*)(links + p0);
            const int4 b = *(const int4*)(links + p0 + 4);
            const int32_t l[kMcPer] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int q = 0; q < kMcPer; ++q) out[q] = value(l[q], p0 + q);
        } else {
#pragma unroll
            for (int q = 0; q < kMcPer; ++q) out[q] = p0 + q < P ? at(p0 + q) : 0.0f;
        }
    }
};

// exclusive prefix over the workgroup of one value per thread; *total = the sum
template <class T>
__device__ __forceinline__ T block_exclusive_scan(T x, T* total) {
    __shared__ T buf[kMcThreads];
    const int t = threadIdx.x;
    buf[t] = x;
    __syncthreads();
    for (int d = 1; d < kMcThreads; d <<= 1) {
        const T y = t >= d ? buf[t - d] : T(0);
        __syncthreads();
        buf[t] += y;
        __syncthreads();
    }
    const T incl = buf[t];
    *total = buf[kMcThreads - 1];
    __syncthreads();
    return incl - x;
}

// crossing mask of lattice point p (value vp): bit a set iff the edge to p + e_a exists and its ends classify differently
template <class Vol>
__device__ __forceinline__ unsigned edge_mask(const Vol& g, uint32_t p, float vp) {
    const uint32_t k = p % g.Z, ij = p / g.Z, j = ij % g.Y, i = ij / g.Y;
    const bool in = mc_inside(vp, g.iso);
    unsigned m = 0;
    if (i + 1 < g.X && mc_inside(g.at(p + g.Y * g.Z), g.iso) != in) m |= 1u;
    if (j + 1 < g.Y && mc_inside(g.at(p + g.Z), g.iso) != in) m |= 2u;
    if (k + 1 < g.Z && mc_inside(g.at(p + 1), g.iso) != in) m |= 4u;
    return m;
}

template <class Vol>
__global__ __launch_bounds__(kMcThreads) void mc_edge_count_kernel(const Vol g, uint16_t* rec, int* tile_count) {
    const uint32_t P = g.X * g.Y * g.Z;
    const uint32_t p0 = blockIdx.x * kMcTile + threadIdx.x * kMcPer;
    float v[kMcPer];
    g.load_run(p0, P, v);
    unsigned m[kMcPer];
    int n = 0;
#pragma unroll
    for (int q = 0; q < kMcPer; ++q) {
        m[q] = p0 + q < P ? edge_mask(g, p0 + q, v[q]) : 0u;
        n += __popc(m[q]);
    }
    int total;
    int off = block_exclusive_scan(n, &total);
#pragma unroll
    for (int q = 0; q < kMcPer; ++q) {
        if (p0 + q < P) rec[p0 + q] = (uint16_t)((off << 3) | m[q]);
        off += __popc(m[q]);
    }
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

// case index of cell c (C order over [X-1, Y-1, Z-1]) and the linear index of its corner 0
template <class Vol>
__device__ __forceinline__ unsigned cell_case(const Vol& g, uint32_t c, uint32_t* p_out) {
    const uint32_t Zc = g.Z - 1, Yc = g.Y - 1;
    const uint32_t ck = c % Zc, cij = c / Zc, cj = cij % Yc, ci = cij / Yc;
    const uint32_t p = (ci * g.Y + cj) * g.Z + ck, YZ = g.Y * g.Z;
    const uint32_t off[8] = {0u, 1u, g.Z, g.Z + 1u, YZ, YZ + 1u, YZ + g.Z, YZ + g.Z + 1u};
    unsigned cs = 0;
#pragma unroll
    for (int v = 0; v < 8; ++v) cs |= mc_inside(g.at(p + off[v]), g.iso) ? (1u << v) : 0u;
    *p_out = p;
    return cs;
}

template <class Vol>
__global__ __launch_bounds__(kMcThreads) void mc_cell_count_kernel(const Vol g, int* tile_count) {
    const uint32_t C = (g.X - 1) * (g.Y - 1) * (g.Z - 1);
    const uint32_t c0 = blockIdx.x * kMcTile + threadIdx.x * kMcPer;
    int n = 0;
    for (int q = 0; q < kMcPer; ++q) {
        if (c0 + q >= C) break;
        uint32_t p;
        n += c_ntri[cell_case(g, c0 + q, &p)];
    }
    int total;
    (void)block_exclusive_scan(n, &total);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

// blockIdx.x selects the array: counts[b][0..n[b]) -> offsets[b] (exclusive, int64), totals[b]
struct ScanJob {
    const int* counts[2];
    int64_t* offsets[2];
    int n[2];
    int64_t* totals;
};

__global__ __launch_bounds__(kMcThreads) void mc_scan_kernel(const ScanJob j) {
    const int b = blockIdx.x;
    const int n = j.n[b];
    const int per = (n + kMcThreads - 1) / kMcThreads;
    const int lo = threadIdx.x * per, hi = lo + per < n ? lo + per : n;
    int64_t s = 0;
    for (int i = lo; i < hi; ++i) s += j.counts[b][i];
    int64_t total;
    int64_t off = block_exclusive_scan(s, &total);
    for (int i = lo; i < hi; ++i) {
        j.offsets[b][i] = off;
        off += j.counts[b][i];
    }
    if (threadIdx.x == 0) j.totals[b] = total;
}

template <class Vol>
__global__ __launch_bounds__(kMcThreads) void mc_vertex_kernel(const Vol g, const uint16_t* rec, const int64_t* tile_off, float* out) {
    const uint32_t P = g.X * g.Y * g.Z;
    const uint32_t p0 = blockIdx.x * kMcTile + threadIdx.x * kMcPer;
    float v[kMcPer];
    g.load_run(p0, P, v);
    const int64_t base = tile_off[blockIdx.x];
    for (int q = 0; q < kMcPer; ++q) {
        const uint32_t p = p0 + q;
        if (p >= P) break;
        const unsigned r = rec[p];
        if (!(r & 7u)) continue;
        int64_t id = base + (r >> 3);
        const uint32_t k = p % g.Z, ij = p / g.Z, j = ij % g.Y, i = ij / g.Y;
        const uint32_t stride[3] = {g.Y * g.Z, g.Z, 1u};
        for (int ax = 0; ax < 3; ++ax) {
            if (!((r >> ax) & 1u)) continue;
            const float a = v[q], b = g.at(p + stride[ax]);
            float t = (g.iso - a) / (b - a);
            if (!(fabsf(t) <= 3.4028234663852886e38f)) t = 0.5f;      // a NaN or infinite end
            float xyz[3] = {(float)i, (float)j, (float)k};
            xyz[ax] = xyz[ax] + t;
            out[id * 3 + 0] = xyz[0];
            out[id * 3 + 1] = xyz[1];
            out[id * 3 + 2] = xyz[2];
            ++id;
        }
    }
}

template <class Vol>
__global__ __launch_bounds__(kMcThreads) void mc_triangle_kernel(const Vol g, const uint16_t* rec, const int64_t* vtile_off,
                                                                 const int64_t* ttile_off, int64_t* out) {
    const uint32_t C = (g.X - 1) * (g.Y - 1) * (g.Z - 1);
    const uint32_t c0 = blockIdx.x * kMcTile + threadIdx.x * kMcPer;
    unsigned cs[kMcPer];
    uint32_t pc[kMcPer];
    int n = 0;
#pragma unroll
    for (int q = 0; q < kMcPer; ++q) {
        cs[q] = 0u;
        pc[q] = 0u;
        if (c0 + q < C) cs[q] = cell_case(g, c0 + q, &pc[q]);
        n += c_ntri[cs[q]];
    }
    int total;
    const int off = block_exclusive_scan(n, &total);
    int64_t t = ttile_off[blockIdx.x] + off;
    const uint32_t YZ = g.Y * g.Z;
    for (int q = 0; q < kMcPer; ++q) {
        const int nt = c_ntri[cs[q]];
        for (int e = 0; e < 3 * nt; ++e) {
            const int edge = c_tri[cs[q]][e];
            const int v = c_edge_corner[edge], ax = c_edge_axis[edge];
            const uint32_t p = pc[q] + ((v >> 2) & 1) * YZ + ((v >> 1) & 1) * g.Z + (v & 1);
            const unsigned r = rec[p];
            out[t * 3 + e] = vtile_off[p / kMcTile] + (r >> 3) + __popc(r & 7u & ((1u << ax) - 1u));
        }
        t += nt;
    }
}

// ---- the triangle table ----------------------------------------------------------------------------------------
// Generated rather than transcribed. For a case (bit v = corner v inside, i.e. v >= iso):
//   * every face of the cube contributes segments between its crossing edges: with two crossings one segment; with four
//     (diagonal corners alike) each INSIDE corner is cut off by its own segment. The rule depends on the face's four corners
//     only, so the two cells that share a face draw the same segments there, and the surface is closed across cells.
//   * a segment is directed so that (d x n) points to the inside corners, n the face's outward normal; every crossing edge
//     then has one incoming and one outgoing segment, and the segments form disjoint directed loops.
//   * each loop is fanned into triangles from the first vertex (in loop order from its lowest edge) whose fan diagonals do
//     not join two vertices of one face: such a diagonal could be drawn by the neighbour across that face too. Every loop
//     of the 256 cases has such a vertex; at most 5 triangles per case.
// The right-hand normal of a triangle then points out of the region v >= iso (checked: one inside corner gives the triangle
// whose normal is (1, 1, 1)), i.e. a closed surface has positive signed volume.
struct TriTable {
    int8_t tri[256][16];
    int8_t ntri[256];
};

static void build_tri_table(TriTable& T) {
    static const int ecorner[12] = {0, 1, 2, 3, 0, 1, 4, 5, 0, 2, 4, 6}, eaxis[12] = {0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2};
    auto corner = [](int v, int a) { return (float)((v >> (2 - a)) & 1); };
    auto edge_of = [&](int a, int b) {
        if (a > b) std::swap(a, b);
        for (int e = 0; e < 12; ++e)
            if (ecorner[e] == a && ecorner[e] + (4 >> eaxis[e]) == b) return e;
        return -1;
    };
    auto mid = [&](int e, float* m) {
        for (int a = 0; a < 3; ++a) m[a] = corner(ecorner[e], a) + (a == eaxis[e] ? 0.5f : 0.0f);
    };
    // faces: axis f, side s; corners in cyclic order; outward normal
    int fcyc[6][4], fedge[6][4];
    float fn[6][3];
    for (int f = 0; f < 3; ++f)
        for (int sd = 0; sd < 2; ++sd) {
            const int F = 2 * f + sd, o0 = f == 0 ? 1 : 0, o1 = f == 2 ? 1 : 2;
            const int uv[4][2] = {{0, 0}, {1, 0}, {1, 1}, {0, 1}};
            for (int q = 0; q < 4; ++q) {
                int c[3];
                c[f] = sd;
                c[o0] = uv[q][0];
                c[o1] = uv[q][1];
                fcyc[F][q] = 4 * c[0] + 2 * c[1] + c[2];
            }
            for (int q = 0; q < 4; ++q) fedge[F][q] = edge_of(fcyc[F][q], fcyc[F][(q + 1) & 3]);
            for (int a = 0; a < 3; ++a) fn[F][a] = a == f ? (sd ? 1.0f : -1.0f) : 0.0f;
        }
    auto share_face = [&](int e0, int e1) {
        for (int F = 0; F < 6; ++F) {
            bool a = false, b = false;
            for (int q = 0; q < 4; ++q) {
                a |= fedge[F][q] == e0;
                b |= fedge[F][q] == e1;
            }
            if (a && b) return true;
        }
        return false;
    };
    memset(&T, -1, sizeof(T));
    for (int cs = 0; cs < 256; ++cs) {
        int next[12];
        for (int e = 0; e < 12; ++e) next[e] = -1;
        auto add_segment = [&](int e0, int e1, const float* side, const float* n) {
            float m0[3], m1[3], d[3], x[3];
            mid(e0, m0);
            mid(e1, m1);
            for (int a = 0; a < 3; ++a) d[a] = m1[a] - m0[a];
            x[0] = d[1] * n[2] - d[2] * n[1];
            x[1] = d[2] * n[0] - d[0] * n[2];
            x[2] = d[0] * n[1] - d[1] * n[0];
            if (x[0] * side[0] + x[1] * side[1] + x[2] * side[2] > 0.0f) next[e0] = e1;
            else next[e1] = e0;
        };
        for (int F = 0; F < 6; ++F) {
            int st[4], ncross = 0;
            for (int q = 0; q < 4; ++q) st[q] = (cs >> fcyc[F][q]) & 1;
            for (int q = 0; q < 4; ++q) ncross += st[q] != st[(q + 1) & 3];
            if (ncross == 2) {
                int e[2], k = 0;
                float side[3] = {0.0f, 0.0f, 0.0f};
                int n_in = 0;
                for (int q = 0; q < 4; ++q) {
                    if (st[q] != st[(q + 1) & 3]) e[k++] = fedge[F][q];
                    n_in += st[q];
                }
                // centroid of the inside corners minus centroid of the outside ones
                for (int q = 0; q < 4; ++q)
                    for (int a = 0; a < 3; ++a)
                        side[a] += corner(fcyc[F][q], a) * (st[q] ? 1.0f / n_in : -1.0f / (4 - n_in));
                add_segment(e[0], e[1], side, fn[F]);
            } else if (ncross == 4) {
                for (int q = 0; q < 4; ++q) {
                    if (!st[q]) continue;
                    const int e0 = fedge[F][(q + 3) & 3], e1 = fedge[F][q];
                    float m0[3], m1[3], side[3];
                    mid(e0, m0);
                    mid(e1, m1);
                    for (int a = 0; a < 3; ++a) side[a] = corner(fcyc[F][q], a) - 0.5f * (m0[a] + m1[a]);
                    add_segment(e0, e1, side, fn[F]);
                }
            }
        }
        bool seen[12] = {};
        int nt = 0;
        for (int e = 0; e < 12; ++e) {
            if (next[e] < 0 || seen[e]) continue;
            int loop[12], n = 0;
            for (int x = e; !seen[x]; x = next[x]) {
                seen[x] = true;
                loop[n++] = x;
            }
            int apex = 0;
            for (; apex < n; ++apex) {
                bool ok = true;
                for (int k = 2; k < n - 1 && ok; ++k) ok = !share_face(loop[apex], loop[(apex + k) % n]);
                if (ok) break;
            }
            for (int k = 1; k + 1 < n; ++k) {
                T.tri[cs][3 * nt + 0] = (int8_t)loop[apex];
                T.tri[cs][3 * nt + 1] = (int8_t)loop[(apex + k) % n];
                T.tri[cs][3 * nt + 2] = (int8_t)loop[(apex + k + 1) % n];
                ++nt;
            }
        }
        T.ntri[cs] = (int8_t)nt;
    }
}

hipError_t upload_tri_table() {
    static std::mutex mu;
    static bool done[64] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> lock(mu);
    if (done[dev]) return hipSuccess;
    static TriTable T;
    static bool built = false;
    if (!built) {
        build_tri_table(T);
        built = true;
    }
    e = hipMemcpyToSymbol(HIP_SYMBOL(c_tri), T.tri, sizeof(T.tri));
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(c_ntri), T.ntri, sizeof(T.ntri));
    if (e == hipSuccess) done[dev] = true;
    return e;
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

size_t mc_scratch_bytes(const int32_t reso[3]) {
    const uint64_t P = (uint64_t)reso[0] * reso[1] * reso[2];
    const uint64_t C = (uint64_t)(reso[0] - 1) * (reso[1] - 1) * (reso[2] - 1);
    const uint64_t nv = (P + kMcTile - 1) / kMcTile, nt = (C + kMcTile - 1) / kMcTile;
    return align256(P * 2) + align256(nv * 4) + align256(nt * 4) + align256(nv * 8) + align256(nt * 8) + align256(16);
}

namespace {

template <class Vol>
hipError_t mc_count(const Vol& g, const int32_t reso[3], char* scratch, int64_t* totals_host, hipStream_t s) {
    hipError_t e = upload_tri_table();
    if (e != hipSuccess) return e;
    const uint64_t P = (uint64_t)g.X * g.Y * g.Z, C = (uint64_t)(g.X - 1) * (g.Y - 1) * (g.Z - 1);
    const unsigned nv = (unsigned)((P + kMcTile - 1) / kMcTile), nt = (unsigned)((C + kMcTile - 1) / kMcTile);
    McScratch w = mc_scratch(reso, scratch);
    hipLaunchKernelGGL(mc_edge_count_kernel<Vol>, dim3(nv), dim3(kMcThreads), 0, s, g, w.rec, w.vcount);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(mc_cell_count_kernel<Vol>, dim3(nt), dim3(kMcThreads), 0, s, g, w.tcount);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const ScanJob j{{w.vcount, w.tcount}, {w.voff, w.toff}, {(int)nv, (int)nt}, w.totals};
    hipLaunchKernelGGL(mc_scan_kernel, dim3(2), dim3(kMcThreads), 0, s, j);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(totals_host, w.totals, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    return hipStreamSynchronize(s);
}

template <class Vol>
hipError_t mc_emit(const Vol& g, const int32_t reso[3], char* scratch, float* vertices, int64_t* triangles, hipStream_t s) {
    const uint64_t P = (uint64_t)g.X * g.Y * g.Z, C = (uint64_t)(g.X - 1) * (g.Y - 1) * (g.Z - 1);
    const unsigned nv = (unsigned)((P + kMcTile - 1) / kMcTile), nt = (unsigned)((C + kMcTile - 1) / kMcTile);
    McScratch w = mc_scratch(reso, scratch);
    hipError_t e;
    hipLaunchKernelGGL(mc_vertex_kernel<Vol>, dim3(nv), dim3(kMcThreads), 0, s, g, w.rec, w.voff, vertices);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(mc_triangle_kernel<Vol>, dim3(nt), dim3(kMcThreads), 0, s, g, w.rec, w.voff, w.toff, triangles);
    return hipGetLastError();
}

McVolume dense_source(const McArgs& m) {
    return McVolume{m.volume, (uint32_t)m.reso[0], (uint32_t)m.reso[1], (uint32_t)m.reso[2], m.iso,
                    (reinterpret_cast<uintptr_t>(m.volume) & 15) == 0 ? 1 : 0};
}

McGridVolume grid_source(const McGridArgs& m) {
    return McGridVolume{m.links, m.density, m.mask, m.capacity, (uint32_t)m.reso[0], (uint32_t)m.reso[1], (uint32_t)m.reso[2],
                        m.iso, (reinterpret_cast<uintptr_t>(m.links) & 15) == 0 ? 1 : 0};
}

}  // namespace

hipError_t launch_mc_count(const McArgs& m, char* scratch, int64_t* totals_host, hipStream_t s) {
    return mc_count(dense_source(m), m.reso, scratch, totals_host, s);
}

hipError_t launch_mc_emit(const McArgs& m, char* scratch, hipStream_t s) {
    return mc_emit(dense_source(m), m.reso, scratch, m.vertices, m.triangles, s);
}

hipError_t launch_grid_mc_count(const McGridArgs& m, char* scratch, int64_t* totals_host, hipStream_t s) {
    return mc_count(grid_source(m), m.reso, scratch, totals_host, s);
}

hipError_t launch_grid_mc_emit(const McGridArgs& m, char* scratch, hipStream_t s) {
    return mc_emit(grid_source(m), m.reso, scratch, m.vertices, m.triangles, s);
}

McScratch mc_scratch(const int32_t reso[3], char* base) {
    const uint64_t P = (uint64_t)reso[0] * reso[1] * reso[2];
    const uint64_t C = (uint64_t)(reso[0] - 1) * (reso[1] - 1) * (reso[2] - 1);
    const uint64_t nv = (P + kMcTile - 1) / kMcTile, nt = (C + kMcTile - 1) / kMcTile;
    McScratch w;
    size_t off = 0;
    w.rec = (uint16_t*)(base + off);
    off += align256(P * 2);
    w.vcount = (int*)(base + off);
    off += align256(nv * 4);
    w.tcount = (int*)(base + off);
    off += align256(nt * 4);
    w.voff = (int64_t*)(base + off);
    off += align256(nv * 8);
    w.toff = (int64_t*)(base + off);
    off += align256(nt * 8);
    w.totals = (int64_t*)(base + off);
    return w;
}

}  // namespace nerf
