// gs360_vidsteps.h -- the per-lane steps of VID-COLOR v1: decoded Y'CbCr planes -> interleaved RGB.
// Host and device: gs360_vidcolor.hip runs them one lane per pixel group with the tables in LDS, tests/tools/vidcolor_hostcheck.hip
// steps them on the host with the tables in plain arrays.  Every float32 operation below is one operation of the spec, in its order
// (the library is built with -ffp-contract=off), so tests/vidcolor_np.py gives the same levels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gs360 {

constexpr int kVcBits = 14;                      // R'G'B' after the integer step: 0 .. 16383
constexpr int kVcLevels = 1 << kVcBits;          // entries of the linearising table
constexpr int kVcShift = 14;                     // fraction bits of the integer coefficients
constexpr int kVcEnc = 1024;                     // cells of the encode table (indexed by sqrt of the linear value)
constexpr int kVcGroup = 8;                      // pixels of a lane's group along a row; a group is two rows high

struct VcCoef {            // the Y'CbCr -> R'G'B' step: round(x * 2^14 * 16383) of the spec's real coefficients
    int32_t cy, crv, cgu, cgv, cbu;
    int32_t yoff, coff;    // 16 s and 128 s (limited range), 0 and 128 s (full range)
    int32_t vmax;          // 2^d - 1: samples above it are clamped to it
};

struct VcTables {
    const float* lin;      // kVcLevels: Rec.709 R'G'B' level -> linear light
    const float2* enc;     // kVcEnc cells: (level at the cell's lower edge, rise over the cell), in output levels
    float m[9];            // BT.709 -> SMPTE-C primaries, row-major
    int32_t outmax;        // 255 or 65535: the destination's largest level
};

struct VcImage {           // one job; strides in bytes
    const uint8_t *y, *cb, *cr;
    uint8_t* dst;
    int64_t ys, cbs, crs, ds;
    int32_t W, H;
    int32_t sx, sy;        // chroma shifts: 4:2:0 = (1, 1), 4:2:2 = (1, 0), 4:4:4 = (0, 0)
    int32_t fast;          // every plane pointer, the destination and all four strides are multiples of 4
    int32_t gpr;           // groups per row, ceil(W / 8)
};

__host__ __device__ inline int vc_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Integer step: samples (clamped to vmax) -> 14-bit R'G'B'.  Every sum stays below 2^31 (the glue derives the coefficients).
__host__ __device__ inline void vc_rgb14(const VcCoef& K, int Y, int U, int V, int (&q)[3]) {
    Y = Y > K.vmax ? K.vmax : Y;
    U = U > K.vmax ? K.vmax : U;
    V = V > K.vmax ? K.vmax : V;
    const int yy = K.cy * (Y - K.yoff) + (1 << (kVcShift - 1));
    const int u = U - K.coff, v = V - K.coff;
    q[0] = vc_clampi((yy + K.crv * v) >> kVcShift, 0, kVcLevels - 1);
    q[1] = vc_clampi((yy - K.cgu * u - K.cgv * v) >> kVcShift, 0, kVcLevels - 1);
    q[2] = vc_clampi((yy + K.cbu * u) >> kVcShift, 0, kVcLevels - 1);
}

// Float step: linearise (table), change primaries, clip, encode (table, linear between cell edges), round.
__host__ __device__ inline void vc_levels(const VcTables& T, const int (&q)[3], int (&o)[3]) {
    const float r = T.lin[q[0]], g = T.lin[q[1]], b = T.lin[q[2]];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float l = (T.m[3 * c] * r + T.m[3 * c + 1] * g) + T.m[3 * c + 2] * b;
        l = fminf(fmaxf(l, 0.0f), 1.0f);
        const float p = sqrtf(l) * (float)kVcEnc;
        int i = (int)p;
        i = i > kVcEnc - 1 ? kVcEnc - 1 : i;
        const float f = p - (float)i;
        const float2 e = T.enc[i];
        o[c] = vc_clampi((int)rintf(e.x + e.y * f), 0, T.outmax);
    }
}

template <typename S>
__host__ __device__ inline const S* vc_row(const uint8_t* base, int64_t stride, int y) {
    return reinterpret_cast<const S*>(base + (int64_t)y * stride);
}

// One pixel through both steps with sample-sized loads and stores: the tail of a row, and every pixel of a job that is not `fast`.
// D: the destination's sample type (uint8_t from uint16_t planes is the (10, 8) format of DESIGN.md section 19).
template <typename S, typename D = S>
__host__ __device__ inline void vc_pixel(const VcImage& I, const VcCoef& K, const VcTables& T, int x, int y) {
    const int cx = x >> I.sx, cy = y >> I.sy;
    int q[3], o[3];
    vc_rgb14(K, (int)vc_row<S>(I.y, I.ys, y)[x], (int)vc_row<S>(I.cb, I.cbs, cy)[cx], (int)vc_row<S>(I.cr, I.crs, cy)[cx], q);
    vc_levels(T, q, o);
    D* d = reinterpret_cast<D*>(I.dst + (int64_t)y * I.ds) + 3 * (int64_t)x;
    d[0] = (D)o[0]; d[1] = (D)o[1]; d[2] = (D)o[2];
}

// N samples of S as whole dwords from a dword-aligned address, and sample i of them
template <typename S, int N>
struct VcWords { uint32_t w[N * (int)sizeof(S) / 4]; };
template <typename S, int N>
__host__ __device__ inline VcWords<S, N> vc_load(const S* p) {
    VcWords<S, N> r;
    __builtin_memcpy(r.w, __builtin_assume_aligned(p, 4), sizeof(r.w));
    return r;
}
template <typename S, int N>
__host__ __device__ inline int vc_sample(const VcWords<S, N>& v, int i) {
    constexpr int kBits = 8 * (int)sizeof(S), kPer = 32 / kBits;
    return (int)((v.w[i / kPer] >> ((i % kPer) * kBits)) & ((1u << kBits) - 1u));
}

// Eight pixels of row y from x0 (x0 + 8 <= W, `fast` job): whole-dword loads, 6 (D = uint8) or 12 (D = uint16) whole-dword stores.
// SX: the chroma planes are subsampled along the row (four samples serve the eight pixels).
template <typename S, int SX, typename D = S>
__host__ __device__ inline void vc_row8(const VcImage& I, const VcCoef& K, const VcTables& T, int x0, int y) {
    constexpr int kBits = 8 * (int)sizeof(D), kPer = 32 / kBits, kC = kVcGroup >> SX, kOut = 3 * kVcGroup / kPer;
    const int cy = y >> I.sy, cx0 = x0 >> SX;
    const VcWords<S, kVcGroup> Y = vc_load<S, kVcGroup>(vc_row<S>(I.y, I.ys, y) + x0);
    const VcWords<S, kC> U = vc_load<S, kC>(vc_row<S>(I.cb, I.cbs, cy) + cx0);
    const VcWords<S, kC> V = vc_load<S, kC>(vc_row<S>(I.cr, I.crs, cy) + cx0);
    uint32_t out[kOut];
#pragma unroll
    for (int j = 0; j < kOut; ++j) out[j] = 0u;
#pragma unroll
    for (int i = 0; i < kVcGroup; ++i) {
        int q[3], o[3];
        vc_rgb14(K, vc_sample<S, kVcGroup>(Y, i), vc_sample<S, kC>(U, i >> SX), vc_sample<S, kC>(V, i >> SX), q);
        vc_levels(T, q, o);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int s = 3 * i + c;
            out[s / kPer] |= (uint32_t)o[c] << ((s % kPer) * kBits);
        }
    }
    D* d = reinterpret_cast<D*>(I.dst + (int64_t)y * I.ds) + 3 * (int64_t)x0;
    __builtin_memcpy(__builtin_assume_aligned(d, 4), out, sizeof(out));
}

// Group g of a job: pixels [8 gx, 8 gx + 8) of rows 2 gy and 2 gy + 1, clipped to the image.
template <typename S, typename D = S>
__host__ __device__ inline void vc_group(const VcImage& I, const VcCoef& K, const VcTables& T, uint32_t g) {
    const int gy = (int)(g / (uint32_t)I.gpr), gx = (int)(g - (uint32_t)gy * (uint32_t)I.gpr);
    const int x0 = gx * kVcGroup;
    const int n = I.W - x0 < kVcGroup ? I.W - x0 : kVcGroup;
#pragma unroll 1
    for (int y = 2 * gy; y < 2 * gy + 2 && y < I.H; ++y) {
        if (I.fast && n == kVcGroup) {
            if (I.sx) vc_row8<S, 1, D>(I, K, T, x0, y);
            else vc_row8<S, 0, D>(I, K, T, x0, y);
        } else {
            for (int i = 0; i < n; ++i) vc_pixel<S, D>(I, K, T, x0 + i, y);
        }
    }
}

inline uint32_t vc_groups(const VcImage& I) { return (uint32_t)I.gpr * (uint32_t)((I.H + 1) / 2); }

constexpr int kVcMaxJobs = 16;                   // GS360_MAX_FRAMES
struct VidLaunch {         // the kernel's argument: a plan's tables (device memory) and the jobs of one call
    const float* lin;
    const float2* enc;
    float m[9];
    int32_t outmax;
    VcCoef coef;
    int32_t n_jobs;
    uint32_t tile_end[kVcMaxJobs];               // tiles of 512 groups up to and including job j (filled by launch_vidcolor)
    VcImage img[kVcMaxJobs];
};
hipError_t launch_vidcolor(VidLaunch& L, int depth, int out_bits, hipStream_t s);   // gs360_vidcolor.hip; n_jobs >= 1, (8, 8), (10, 16) or (10, 8)

}  // namespace gs360
