// gs360_vidfishsteps.h -- the per-lane steps of VID-FISHEYE v1: the planes of a decoded fisheye frame -> an
// S x S pinhole view in RGB.  Coordinate, weights, tap sums and visibility; the colour steps are VID-COLOR v1's (gs360_vidsteps.h).
// Host and device: gs360_vidfisheye.hip runs them one lane per output pixel with the tables in LDS, tests/tools/vidfisheye_hostcheck.hip
// steps them on the host.  Every float32 operation below is one operation of the spec, in its order, and none is fused (the library
// is built with -ffp-contract=off and nothing here calls fma), so tests/vidfisheye_np.py gives the same bytes.  `/` and sqrtf are the
// correctly rounded forms on both sides (-fhip-fp32-correctly-rounded-divide-sqrt); eq_div / eq_sqrt are device-only and their
// documented domain (section 18.2) would hold, but a header the host steps cannot call them.
#pragma once
#include "gs360_eqspec.h"
#include "gs360_vidsteps.h"

namespace gs360 {

constexpr int kVfEquidistant = 0, kVfEquisolid = 1;      // GS360_FISHEYE_*
constexpr int kVfPhases = 32;                            // 1/32 px
constexpr int kVfOne = 16384;                            // the weights of a phase sum to this
constexpr int kVfTileW = 32, kVfTileH = 16;              // output pixels of a workgroup tile; a wavefront takes 16 x 4 of them
constexpr float kVfPi4 = 0x1.921fb6p-1f;                 // f32(pi / 4)
constexpr float kVfLimit = 16777216.0f;                  // 2^24: coordinates are clamped to it before they become integers

struct VfView {            // the float32 constants of a call (the glue derives them in float64, rounded once)
    int32_t proj;          // kVfEquidistant | kVfEquisolid
    int32_t S;             // the view is S x S
    float tx, ty;          // tan(fov / 2) / S
    float kx32, ky32;      // 32 kx, 32 ky: full-resolution axis, 1/32 px per unit of x g
    float kx16, ky16;      // 16 kx, 16 ky: an axis subsampled by two
    float ox32, oy32;      // 16 W - 16, 16 H - 16
    float ox16, oy16;      // 8 W - 16, 8 H - 16
};

struct VfCoord {
    int sx, sy;            // luma coordinate, 1/32 px
    int cx, cy;            // coordinate on an axis subsampled by two (valid where the job subsamples that axis)
    bool visible;
};

// atan(h), h >= 0: EQ-SPEC's octant reduction of atan2(h, 1) and its degree-4 polynomial, Horner with separate multiply and add
__host__ __device__ inline float vf_atan(float h) {
    const bool steep = h > 1.0f;
    const float mx = steep ? h : 1.0f, mn = steep ? 1.0f : h;
    const bool big = mn > EQ_T8 * mx;
    const float num = big ? mn - mx : mn;
    const float den = big ? mn + mx : mx;
    const float t = num / den;
    const float z = t * t;
    float p = EQ_C5 * z + EQ_C4;
    p = p * z + EQ_C3;
    p = p * z + EQ_C2;
    p = p * z + EQ_C1;
    float r0 = (p * z) * t + t;
    int k = big ? 1 : 0;
    if (steep) { r0 = -r0; k = 2 - k; }
    return (float)k * kVfPi4 + r0;
}

// g with (x g, y g) the direction in the fisheye image, in units of the lens constant
__host__ __device__ inline float vf_gain(int proj, float q) {
    if (proj == kVfEquisolid) {
        const float n = sqrtf(1.0f + q);
        const float d = (2.0f * n) * (n + 1.0f);
        return 1.0f / sqrtf(d);
    }
    const float h = sqrtf(q);
    const float th = vf_atan(h);
    return h > 0.0f ? th / h : 1.0f;
}

__host__ __device__ inline int vf_quant(float a, float k, float o) {
    const float v = a * k + o;
    return (int)rintf(fminf(fmaxf(v, -kVfLimit), kVfLimit));
}

__host__ __device__ inline VfCoord vf_coord(const VfView& V, int W, int H, int i, int j) {
    const float x = (float)(2 * i + 1 - V.S) * V.tx, y = (float)(2 * j + 1 - V.S) * V.ty;
    const float q = x * x + y * y;
    const float g = vf_gain(V.proj, q);
    const float xg = x * g, yg = y * g;
    VfCoord c;
    c.sx = vf_quant(xg, V.kx32, V.ox32);
    c.sy = vf_quant(yg, V.ky32, V.oy32);
    c.cx = vf_quant(xg, V.kx16, V.ox16);
    c.cy = vf_quant(yg, V.ky16, V.oy16);
    c.visible = c.sx >= -16 && c.sx < 32 * W - 16 && c.sy >= -16 && c.sy < 32 * H - 16;
    return c;
}

// The four 14-bit weights of phase f: v360's cubic (Lagrange) in integers, round half to even, the residue on the nearer centre tap
__host__ __device__ inline void vf_weights(int f, int16_t* w) {
    const int f2 = f * f, f3 = f2 * f;
    const int N[4] = {-2048 * f + 96 * f2 - f3, 196608 - 3072 * f - 192 * f2 + 3 * f3, 6144 * f + 96 * f2 - 3 * f3, -1024 * f + f3};
    int sum = 0;
    for (int k = 0; k < 4; ++k) {
        int q = N[k] / 12, r = N[k] - 12 * q;
        if (r < 0) { r += 12; --q; }                     // floor
        if (r > 6 || (r == 6 && (q & 1))) ++q;
        w[k] = (int16_t)q;
        sum += q;
    }
    w[f <= 16 ? 1 : 2] += (int16_t)(kVfOne - sum);
}

__host__ __device__ inline int64_t vf_row_sum(const int16_t* wx, int vmax, int a, int b, int c, int d) {
    a = a > vmax ? vmax : a; b = b > vmax ? vmax : b; c = c > vmax ? vmax : c; d = d > vmax ? vmax : d;
    return (int64_t)(wx[0] * a + wx[1] * b + wx[2] * c + wx[3] * d);
}

// One plane of `pw` x `ph` samples at (cx, cy), 1/32 px.  `dword`: the plane's pointer and stride are multiples of 4, so a window
// that lies inside the plane, and whose aligned dwords lie inside its rows, is fetched as 2 (uint8) or 3 (uint16) dwords per row.
template <typename S>
__host__ __device__ inline int vf_plane(const uint8_t* base, int64_t stride, int pw, int ph, int cx, int cy, bool dword,
                                        const int16_t* wtab, int vmax) {
    constexpr int kB = (int)sizeof(S), kND = kB == 1 ? 2 : 3;
    const int ix = cx >> 5, iy = cy >> 5;
    const int16_t* wx = wtab + 4 * (cx & 31);
    const int16_t* wy = wtab + 4 * (cy & 31);
    const int o = (ix - 1) * kB, a = o & ~3;
    int64_t v = 0;
    if (dword && ix >= 1 && ix + 2 < pw && iy >= 1 && iy + 2 < ph && a + 4 * kND <= pw * kB) {
        const uint8_t* p = base + (int64_t)(iy - 1) * stride + a;
        const int sh = (o - a) * 8;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            uint32_t d[kND];
            __builtin_memcpy(d, __builtin_assume_aligned(p + (int64_t)m * stride, 4), sizeof(d));
            const uint32_t lo = (uint32_t)((((uint64_t)d[1] << 32) | d[0]) >> sh);
            int64_t r;
            if constexpr (kB == 1) {
                r = vf_row_sum(wx, vmax, (int)(lo & 255u), (int)((lo >> 8) & 255u), (int)((lo >> 16) & 255u), (int)(lo >> 24));
            } else {
                const uint32_t hi = (uint32_t)((((uint64_t)d[2] << 32) | d[1]) >> sh);
                r = vf_row_sum(wx, vmax, (int)(lo & 65535u), (int)(lo >> 16), (int)(hi & 65535u), (int)(hi >> 16));
            }
            v += (int64_t)wy[m] * r;
        }
    } else {
        const int c0 = vc_clampi(ix - 1, 0, pw - 1), c1 = vc_clampi(ix, 0, pw - 1);
        const int c2 = vc_clampi(ix + 1, 0, pw - 1), c3 = vc_clampi(ix + 2, 0, pw - 1);
#pragma unroll 1
        for (int m = 0; m < 4; ++m) {
            const S* row = vc_row<S>(base, stride, vc_clampi(iy - 1 + m, 0, ph - 1));
            v += (int64_t)wy[m] * vf_row_sum(wx, vmax, (int)row[c0], (int)row[c1], (int)row[c2], (int)row[c3]);
        }
    }
    return vc_clampi((int)((v + ((int64_t)1 << 27)) >> 28), 0, vmax);
}

// Output pixel (i, j) of a job: I.W x I.H is the source, I.dst the S x S x 3 view, I.fast says that the three plane pointers and
// strides are multiples of 4.  The destination is written sample by sample.
template <typename S>
__host__ __device__ inline void vf_pixel(const VcImage& I, const VfView& V, const VcCoef& K, const VcTables& T, const int16_t* wtab,
                                         int i, int j) {
    const VfCoord c = vf_coord(V, I.W, I.H, i, j);
    int o[3] = {0, 0, 0};
    if (c.visible) {
        const int cw = (I.W + I.sx) >> I.sx, ch = (I.H + I.sy) >> I.sy;
        const int ux = I.sx ? c.cx : c.sx, uy = I.sy ? c.cy : c.sy;
        const int Y = vf_plane<S>(I.y, I.ys, I.W, I.H, c.sx, c.sy, I.fast != 0, wtab, K.vmax);
        const int U = vf_plane<S>(I.cb, I.cbs, cw, ch, ux, uy, I.fast != 0, wtab, K.vmax);
        const int Vv = vf_plane<S>(I.cr, I.crs, cw, ch, ux, uy, I.fast != 0, wtab, K.vmax);
        int q[3];
        vc_rgb14(K, Y, U, Vv, q);
        vc_levels(T, q, o);
    }
    S* d = reinterpret_cast<S*>(I.dst + (int64_t)j * I.ds) + 3 * (int64_t)i;
    d[0] = (S)o[0]; d[1] = (S)o[1]; d[2] = (S)o[2];
}

struct VfLaunch {          // the kernel's argument
    const float* lin;
    const float2* enc;
    float m[9];
    int32_t outmax;
    VcCoef coef;
    VfView view;
    int32_t n_jobs;
    int32_t tiles_x, tiles_y;                            // tiles of kVfTileW x kVfTileH per job (filled by launch_vidfisheye)
    VcImage img[kVcMaxJobs];
};
hipError_t launch_vidfisheye(VfLaunch& L, int depth, hipStream_t s);   // gs360_vidfisheye.hip; n_jobs >= 1

}  // namespace gs360
