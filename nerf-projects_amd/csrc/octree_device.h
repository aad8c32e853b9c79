// PlenOctree (nerf_mi355x.h, "PlenOctree"): the device functions of the march that the renderer (octree_kernels.hip) and its
// backward (octree_grad_kernels.hip) share - the SH basis, unit(p), a ray's set-up, the descent, the activation and the image
// form's tile. Both kernels run these very operations, so that the backward's replay of a march gives the renderer's bits.
#pragma once
#include <type_traits>

#include "grid_device.h"
#include "octree_internal.h"

namespace nerf {
namespace {

constexpr int kTile = 8;

template <class F>
hipError_t dispatch_octree_basis(int basis_dim, F&& f) {
    switch (basis_dim) {
        case 1: return f(std::integral_constant<int, 1>());
        case 4: return f(std::integral_constant<int, 4>());
        case 9: return f(std::integral_constant<int, 9>());
        case 16: return f(std::integral_constant<int, 16>());
        case 25: return f(std::integral_constant<int, 25>());
    }
    return hipErrorInvalidValue;
}

// the B basis values at (x, y, z): the reference's sh.py, fp32, each operation rounded, left to right
template <int B>
__device__ __forceinline__ void octree_sh_basis(float x, float y, float z, float (&b)[B]) {
    b[0] = 0.28209479177387814f;
    if (B > 1) {
        b[1 % B] = mul(-0.4886025119029199f, y);
        b[2 % B] = mul(0.4886025119029199f, z);
        b[3 % B] = mul(-0.4886025119029199f, x);
    }
    const float xx = mul(x, x), yy = mul(y, y), zz = mul(z, z);
    const float xy = mul(x, y), yz = mul(y, z), xz = mul(x, z);
    if (B > 4) {
        b[4 % B] = mul(1.0925484305920792f, xy);
        b[5 % B] = mul(-1.0925484305920792f, yz);
        b[6 % B] = mul(0.31539156525252005f, sub(sub(mul(2.0f, zz), xx), yy));
        b[7 % B] = mul(-1.0925484305920792f, xz);
        b[8 % B] = mul(0.5462742152960396f, sub(xx, yy));
    }
    if (B > 9) {
        b[9 % B] = mul(mul(-0.5900435899266435f, y), sub(mul(3.0f, xx), yy));
        b[10 % B] = mul(mul(2.890611442640554f, xy), z);
        b[11 % B] = mul(mul(-0.4570457994644658f, y), sub(sub(mul(4.0f, zz), xx), yy));
        b[12 % B] = mul(mul(0.3731763325901154f, z), sub(sub(mul(2.0f, zz), mul(3.0f, xx)), mul(3.0f, yy)));
        b[13 % B] = mul(mul(-0.4570457994644658f, x), sub(sub(mul(4.0f, zz), xx), yy));
        b[14 % B] = mul(mul(1.445305721320277f, z), sub(xx, yy));
        b[15 % B] = mul(mul(-0.5900435899266435f, x), sub(xx, mul(3.0f, yy)));
    }
    if (B > 16) {
        b[16 % B] = mul(mul(2.5033429417967046f, xy), sub(xx, yy));
        b[17 % B] = mul(mul(-1.7701307697799304f, yz), sub(mul(3.0f, xx), yy));
        b[18 % B] = mul(mul(0.9461746957575601f, xy), sub(mul(7.0f, zz), 1.0f));
        b[19 % B] = mul(mul(-0.6690465435572892f, yz), sub(mul(7.0f, zz), 3.0f));
        b[20 % B] = mul(0.10578554691520431f, add(mul(zz, sub(mul(35.0f, zz), 30.0f)), 3.0f));
        b[21 % B] = mul(mul(-0.6690465435572892f, xz), sub(mul(7.0f, zz), 3.0f));
        b[22 % B] = mul(mul(0.47308734787878004f, sub(xx, yy)), sub(mul(7.0f, zz), 1.0f));
        b[23 % B] = mul(mul(-1.7701307697799304f, xz), sub(xx, mul(3.0f, yy)));
        b[24 % B] = mul(0.6258357354491761f, sub(mul(xx, sub(xx, mul(3.0f, yy))), mul(yy, sub(mul(3.0f, xx), yy))));
    }
}

// unit(p) of the header: where the line p + t d enters and leaves the unit cube
__device__ __forceinline__ void unit_cube(const float p[3], const float inv[3], float& tmin, float& tmax) {
    tmin = 0.0f;
    tmax = 1e9f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float t1 = mul(-p[i], inv[i]);
        const float t2 = add(t1, inv[i]);
        tmin = fmaxf(tmin, fminf(t1, t2));
        tmax = fminf(tmax, fmaxf(t1, t2));
    }
}

__device__ __forceinline__ float octree_act(int act, float s) {
    return act == NERF_OCTREE_RGB_RELU_HALF ? fmaxf(add(s, 0.5f), 0.0f) : __fdiv_rn(1.0f, add(1.0f, expf(-s)));
}

// the pixel of this thread in row-major order, or -1 outside the image
__device__ __forceinline__ int64_t tile_pixel(const GridCam& cam, int64_t tid) {
    const int64_t tile = tid / (kTile * kTile);
    const int lane = (int)(tid % (kTile * kTile));
    const int tiles_x = (cam.width + kTile - 1) / kTile;
    const int64_t px = (tile % tiles_x) * kTile + lane % kTile;
    const int64_t py = (tile / tiles_x) * kTile + lane / kTile;
    return px < cam.width && py < cam.height ? py * cam.width + px : -1;
}

int64_t image_threads(const GridCam& cam) {
    return (int64_t)((cam.width + kTile - 1) / kTile) * ((cam.height + kTile - 1) / kTile) * (kTile * kTile);
}

// one ray's set-up: the header's o, d, inv, delta_scale and unit(o)
struct OctreeRay {
    float o[3], d[3], inv[3];
    float delta_scale, tmin, tmax;
    bool ok;
};

__device__ __forceinline__ void octree_setup(const OctreeDev& t, const float ow[3], const float dw[3], OctreeRay& r) {
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        finite = finite && isfinite(ow[i]) && isfinite(dw[i]);
        r.o[i] = add(mul(ow[i], t.invradius[i]), t.offset[i]);
        r.d[i] = mul(dw[i], t.invradius[i]);
    }
    const float n = sqrtf(add(add(mul(r.d[0], r.d[0]), mul(r.d[1], r.d[1])), mul(r.d[2], r.d[2])));
    r.delta_scale = __fdiv_rn(1.0f, n);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        r.d[i] = mul(r.d[i], r.delta_scale);
        r.inv[i] = __fdiv_rn(1.0f, add(r.d[i], 1e-9f));
    }
    r.ok = finite && isfinite(r.delta_scale) && r.delta_scale > 0.0f;
    unit_cube(r.o, r.inv, r.tmin, r.tmax);
}

// the leaf that holds p (in the unit cube, changed to the position inside the leaf): its cell index; inv_cube = 1 / cube.
// ACCEL: the descent starts at the table's cell instead of the root. With q = p 2^d, the position inside the cell of depth d
// is q - floor(q): the d doublings and subtractions of the plain descent are exact in fp32, so this is the number they give,
// and the leaf, the position and inv_cube are the plain descent's, bit for bit.
template <bool ACCEL>
__device__ __forceinline__ int64_t octree_descend(const OctreeDev& t, float p[3], float& inv_cube) {
    int64_t node = 0, cell = 0;
    int depth = 0;
    inv_cube = 1.0f;
    if (ACCEL) {
        const int k = t.table_levels;
        const float side = (float)(1 << k);
        const int ix = (int)mul(p[0], side), iy = (int)mul(p[1], side), iz = (int)mul(p[2], side);      // p < 1: below 2^k
        const int2 e = t.table[(((((int64_t)ix << k) + iy) << k)) + iz];
        cell = e.x;
        const float scale = (float)(1 << e.y);
        inv_cube = __fdiv_rn(1.0f, scale);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float q = mul(p[i], scale);
            p[i] = sub(q, floorf(q));
        }
        if (e.y < k) return cell;      // a leaf above the table's level
        const int32_t skip = t.child[cell];
        if (skip == 0) return cell;
        node = cell / 8 + skip;
        depth = k;
    }
    for (; depth <= t.max_depth; ++depth) {
        int u[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            p[i] = mul(p[i], 2.0f);
            u[i] = p[i] >= 1.0f ? 1 : 0;      // floor of a value in [0, 2)
            p[i] = sub(p[i], (float)u[i]);
        }
        inv_cube = mul(inv_cube, 0.5f);
        cell = node * 8 + (u[0] * 4 + u[1] * 2 + u[2]);
        const int32_t skip = t.child[cell];
        if (skip == 0) break;
        node += skip;
    }
    return cell;
}

}  // namespace
}  // namespace nerf
