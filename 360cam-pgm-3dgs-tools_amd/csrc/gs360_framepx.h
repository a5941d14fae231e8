// gs360_framepx.h -- FS-SPEC's per-pixel steps, shared by the FrameSelector passes (gs360_framescore.hip, gs360_framefft.hip,
// gs360_frameflow.hip).  Private to those files; the mask kernels (gs360_maskplane.h) take gray_of, the library's one 8-bit gray, and wave_sum from here.
#pragma once
#include "gs360_kernels.h"

namespace gs360 {

// Sample k of the pixel at byte address p.  A uint16 sample is in host byte order; memcpy keeps a row that starts at an odd byte
// address (a padded odd stride) legal.
template <typename T>
__host__ __device__ __forceinline__ int sample_of(const uint8_t* p, int k) {
    if constexpr (sizeof(T) == 1) {
        return p[k];
    } else {
        T v;
        __builtin_memcpy(&v, p + k * (int)sizeof(T), sizeof(T));
        return v;
    }
}

// The gray at full depth: cv2 COLOR_BGR2GRAY has the same coefficients for 8U and 16U; 65535 * 16384 + 8192 < 2^31.
template <int C, typename T = uint8_t>
__host__ __device__ __forceinline__ int gray_of(const uint8_t* p, int red) {
    if constexpr (C == 1) {
        return sample_of<T>(p, 0);
    } else {
        const int r = sample_of<T>(p, red), g = sample_of<T>(p, 1), b = sample_of<T>(p, 2 - red);
        return (r * 4899 + g * 9617 + b * 1868 + 8192) >> 14;    // cv2 COLOR_BGR2GRAY on 8U / 16U (yuv_shift 14)
    }
}

// The gray of the 8-bit view (FS-DEPTH16 v1, edge and flow passes): every sample >> 8 of a 16-bit pixel, then the 8-bit gray.
template <int C, typename T>
__host__ __device__ __forceinline__ int gray8_of(const uint8_t* p, int red) {
    if constexpr (sizeof(T) == 1) {
        return gray_of<C>(p, red);
    } else if constexpr (C == 1) {
        return sample_of<T>(p, 0) >> 8;
    } else {
        const int r = sample_of<T>(p, red) >> 8, g = sample_of<T>(p, 1) >> 8, b = sample_of<T>(p, 2 - red) >> 8;
        return (r * 4899 + g * 9617 + b * 1868 + 8192) >> 14;
    }
}

// FS-DEPTH16 v1's constants on the 16-bit gray g16, in units of 1/257 gray level (255 / 65535 = 1 / 257)
constexpr int kFs16Highlight = 62259;       // the smallest g16 with g16 / 257 >= 0.95 * 255 = 242.25
// The gray as the fft input's float32: the 8-bit gray itself, or the reference's float32 product g16 * float32(255 / 65535).
template <int C, typename T>
__host__ __device__ __forceinline__ float gray_f32(const uint8_t* p, int red) {
    if constexpr (sizeof(T) == 1) return (float)gray_of<C>(p, red);
    else return (float)gray_of<C, T>(p, red) * (float)(255.0 / 65535.0);
}
// The gray as plane 1 of the fft input holds it, an integer 8-bit level whose `>= 243` is the highlight test: floor(g16 / 257 + 0.75).
template <int C, typename T>
__host__ __device__ __forceinline__ float gray_level(const uint8_t* p, int red) {
    if constexpr (sizeof(T) == 1) return (float)gray_of<C>(p, red);
    else return (float)((gray_of<C, T>(p, red) + 192) / 257);
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One axis of cv::computeResizeAreaTab for output index d: source cells [i1, i2) of weight `mid`, plus a leading cell i1-1 of
// weight `head` and a trailing cell i2 of weight `tail` when those flags are set.
struct AreaSpan {
    int i1, i2;
    bool has_head, has_tail;
    float head, mid, tail;
};
__device__ __forceinline__ AreaSpan area_span(int d, int ssize, double scale) {
    const double f1 = d * scale, f2 = f1 + scale;
    const double cell = fmin(scale, ssize - f1);
    int s2 = (int)floor(f2), s1 = (int)ceil(f1);
    s2 = min(s2, ssize - 1);
    s1 = min(s1, s2);
    AreaSpan a;
    a.i1 = s1;
    a.i2 = s2;
    a.has_head = s1 - f1 > 1e-3;
    a.head = (float)((s1 - f1) / cell);
    a.mid = (float)(1.0 / cell);
    a.has_tail = f2 - s2 > 1e-3;
    a.tail = (float)(fmin(fmin(f2 - s2, 1.0), cell) / cell);
    return a;
}

// The gray of one row's output pixel along x: buf[dx] += S[sx] * alpha, in xtab order.  kView8: the 8-bit view of the samples (the
// flow pass), else the gray at full depth scaled to [0, 255] (the fft input).
template <int C, typename T = uint8_t, bool kView8 = false>
__device__ __forceinline__ float area_row(const uint8_t* row, const AreaSpan& ax, int red) {
    constexpr int kPx = C * (int)sizeof(T);
    auto gray = [&](int sx) { return kView8 ? (float)gray8_of<C, T>(row + sx * kPx, red) : gray_f32<C, T>(row + sx * kPx, red); };
    float buf = 0.0f;
    if (ax.has_head) buf += gray(ax.i1 - 1) * ax.head;
    for (int sx = ax.i1; sx < ax.i2; ++sx) buf += gray(sx) * ax.mid;
    if (ax.has_tail) buf += gray(ax.i2) * ax.tail;
    return buf;
}

// INTER_NEAREST (resizeNN): floor(d * scale), scale = 1 / (dsize / ssize), clamped to the last source index
__device__ __forceinline__ int nearest_index(int d, double scale, int ssize) { return min((int)floor(d * scale), ssize - 1); }

// The full-frame circle: (2x - (W-1))^2 + (2y - (H-1))^2 <= 4 r^2, r = max(1, min(W, H) / 2); this is 4 r^2
__device__ __forceinline__ int64_t circle_r4(int W, int H) {
    const int64_t mwh = min(W, H);
    return max((int64_t)4, mwh * mwh);
}

}  // namespace gs360
