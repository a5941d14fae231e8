// gs360_cvremap.h -- what the cv2.remap family shares: the coordinate conversion, the tile order of a batched launch, the straight-line
// bilinear sampler (BORDER_CONSTANT) and the launchers' dispatch.  Used by the table and fused-fisheye kernels (gs360_table.hip), the
// LDS-staged table kernel (gs360_tablestage.hip) and the 16-bit table kernel (gs360_u16.hip).  DF:2001-2008 / DF:1198-1205 are the call sites.
#pragma once
#include "gs360_sampler.h"

namespace gs360 {

__device__ __forceinline__ int cv_round(float v) {  // SSE cvtss2si: half-to-even, indefinite -> INT_MIN
    if (!(v >= -2147483648.0f && v < 2147483648.0f)) return (int)0x80000000;
    return (int)__builtin_rintf(v);
}
__device__ __forceinline__ int sat_s16(int v) { return min(max(v, -32768), 32767); }

// The tile order of a batched launch (table jobs or fisheye views): position b (blockIdx.x, or a step of the persistent walk) -> tile
// number, >= total_tiles past the last tile.  XCD x (= b % 8) walks tiles [x chunk, (x + 1) chunk).
__device__ __forceinline__ int table_tile_order(const int chunk, const int b) { return (b & 7) * chunk + (b >> 3); }
// Tile t < total_tiles: its job / view and its row / column of tiles there.  The job comes back as a pointer into the kernel argument:
// a copy spills the argument array to scratch memory (see fe_views_tile), and an index that the caller looks up again is a second
// address computation.
template <typename Item>
struct TableTile { const Item* item; int tile_y, tile_x; };
template <typename Item>
__device__ __forceinline__ TableTile<Item> table_tile_at(const Item (&item)[GS360_MAX_VIEWS], const int n, int t) {
    int j = 0;
    while (j + 1 < n && t >= item[j + 1].tile_base) ++j;
    TableTile<Item> T;
    T.item = &item[j];
    t -= T.item->tile_base;
    const int tiles_x = T.item->tiles_x;
    T.tile_y = t / tiles_x;
    T.tile_x = t - T.tile_y * tiles_x;
    return T;
}

template <int C>
__device__ __forceinline__ void cv_sample_linear(const uint8_t* __restrict__ src, int64_t stride, int W, int H,
                                                 float mx, float my, const uint8_t (&cval)[4], uint32_t (&out)[4]) {
    // Straight-line formulation (single exit): taps are fetched from clamped, always-valid addresses and
    // replaced by the border constant afterwards, exactly reproducing remapBilinear's BORDER_CONSTANT rule.
    int sx = cv_round(mx * 32.0f), sy = cv_round(my * 32.0f);
    int fx = sx & 31, fy = sy & 31;
    int ix = sat_s16(sx >> 5), iy = sat_s16(sy >> 5);
    bool outside = ix >= W || ix + 1 < 0 || iy >= H || iy + 1 < 0;
    uint32_t a0 = 32 - fx, a1 = fx, b0 = 32 - fy, b1 = fy;
    uint32_t w00 = a0 * b0, w01 = a1 * b0, w10 = a0 * b1, w11 = a1 * b1;
    bool x0in = (unsigned)ix < (unsigned)W, x1in = (unsigned)(ix + 1) < (unsigned)W;
    bool y0in = (unsigned)iy < (unsigned)H, y1in = (unsigned)(iy + 1) < (unsigned)H;
    int xa = min(max(ix, 0), W - 1), xb = min(max(ix + 1, 0), W - 1);
    int ya = min(max(iy, 0), H - 1), yb = min(max(iy + 1, 0), H - 1);
    const uint8_t* ra = src + (int64_t)ya * stride;
    const uint8_t* rb = src + (int64_t)yb * stride;
    uint32_t s00[4], s01[4], s10[4], s11[4];
    bool wide = false;
    if constexpr (C == 3) wide = x0in && y0in && ix < W - 2 && y1in;  // 8-byte reads stay inside the buffer
    if (wide) {
        uint2 t0 = ld_u64(ra + 3 * xa), t1 = ld_u64(rb + 3 * xa);
        s00[0] = byte_of(t0.x, 0); s00[1] = byte_of(t0.x, 1); s00[2] = byte_of(t0.x, 2);
        s01[0] = byte_of(t0.x, 3); s01[1] = byte_of(t0.y, 0); s01[2] = byte_of(t0.y, 1);
        s10[0] = byte_of(t1.x, 0); s10[1] = byte_of(t1.x, 1); s10[2] = byte_of(t1.x, 2);
        s11[0] = byte_of(t1.x, 3); s11[1] = byte_of(t1.y, 0); s11[2] = byte_of(t1.y, 1);
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            s00[c] = ra[xa * C + c]; s01[c] = ra[xb * C + c];
            s10[c] = rb[xa * C + c]; s11[c] = rb[xb * C + c];
        }
    }
    bool in00 = x0in && y0in, in01 = x1in && y0in, in10 = x0in && y1in, in11 = x1in && y1in;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        uint32_t cv = cval[c];
        uint32_t v = blend(in00 ? s00[c] : cv, in01 ? s01[c] : cv, in10 ? s10[c] : cv, in11 ? s11[c] : cv,
                           w00, w01, w10, w11);
        out[c] = outside ? cv : v;
    }
}

// Host: the family's kernels are instantiated per channel count and interpolation -- launch(c, interp) is called with the pair as
// std::integral_constant values (decltype(c)::value is the template argument).
template <typename Launch>
hipError_t launch_c_interp(const int C, const int interp, Launch launch) {
    const auto with_c = [&](auto c) {
        switch (interp) {
            case GS360_INTERP_NEAREST: launch(c, std::integral_constant<int, GS360_INTERP_NEAREST>()); break;
            case GS360_INTERP_LINEAR: launch(c, std::integral_constant<int, GS360_INTERP_LINEAR>()); break;
            case GS360_INTERP_CUBIC: launch(c, std::integral_constant<int, GS360_INTERP_CUBIC>()); break;
            case GS360_INTERP_LANCZOS4: launch(c, std::integral_constant<int, GS360_INTERP_LANCZOS4>()); break;
            default: return hipErrorInvalidValue;
        }
        return hipGetLastError();
    };
    switch (C) {
        case 1: return with_c(std::integral_constant<int, 1>());
        case 3: return with_c(std::integral_constant<int, 3>());
        case 4: return with_c(std::integral_constant<int, 4>());
        default: return hipErrorInvalidValue;
    }
}

}  // namespace gs360
