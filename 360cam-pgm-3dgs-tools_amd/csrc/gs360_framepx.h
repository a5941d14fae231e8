// gs360_framepx.h -- FS-SPEC's per-pixel steps, shared by the FrameSelector passes (gs360_framescore.hip, gs360_framefft.hip,
// gs360_frameflow.hip).  Private to those files; the mask kernels (gs360_maskplane.h) take gray_of, the library's one 8-bit gray, and wave_sum from here.
#pragma once
#include "gs360_kernels.h"

namespace gs360 {

template <int C>
__host__ __device__ __forceinline__ int gray_of(const uint8_t* p, int red) {
    if constexpr (C == 1) {
        return p[0];
    } else {
        const int r = p[red], g = p[1], b = p[2 - red];
        return (r * 4899 + g * 9617 + b * 1868 + 8192) >> 14;    // cv2 COLOR_BGR2GRAY on 8U (yuv_shift 14)
    }
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

// The gray of one row's output pixel along x: buf[dx] += S[sx] * alpha, in xtab order
template <int C>
__device__ __forceinline__ float area_row(const uint8_t* row, const AreaSpan& ax, int red) {
    float buf = 0.0f;
    if (ax.has_head) buf += (float)gray_of<C>(row + (ax.i1 - 1) * C, red) * ax.head;
    for (int sx = ax.i1; sx < ax.i2; ++sx) buf += (float)gray_of<C>(row + sx * C, red) * ax.mid;
    if (ax.has_tail) buf += (float)gray_of<C>(row + ax.i2 * C, red) * ax.tail;
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
