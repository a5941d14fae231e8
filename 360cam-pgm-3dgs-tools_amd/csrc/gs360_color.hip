// gs360_color.hip -- the dual-fisheye tool's input colour stage on the GPU (include/gs360.h, "input colour stage").
//
// Reference: apply_input_color_pipeline, cli_tools/gs360_DualFisheyeDistortionCalibration.py:684-725 --
// u8 -> float01 (DF:603-613) -> .cube trilinear (DF:620-681) -> rec709_to_srgb (DF:565-600, optional) -> u8 (DF:616-618).
// The two scalar ends (level -> grid position, LUT output -> 8-bit level) arrive as host-built tables (256 x 3 floats
// and 255 thresholds, see the header); the interpolation in between is done here in the reference's float32
// operation order (sub, mul, add -- never fused: the library is built with -ffp-contract=off), so the result is the
// byte the NumPy pipeline produces.
//
// Layout.  The red channel has only 256 possible grid positions, so the first of the three interpolation stages
// (along red, DF:672-675) is evaluated once per plan for every (blue node, green node, red LEVEL) with exactly the
// reference's operations.  The results are stored CELL-major: for every (blue cell, green cell, red level) the four
// corners the green and blue stages need -- c00, c10, c01, c11, float3 each -- sit next to each other in one 64-byte
// entry (48 bytes used; n*n*256 entries: 17.8 MB for a 33^3 cube, Infinity-Cache resident).  A pixel then reads ONE
// aligned 48-byte piece of one cache line instead of four 12-byte pieces from four table rows (round 3: the stage ran at
// 0.18 of the roofline on a smooth image and 0.04 on noise, where every pixel pulled four lines).  The output quantiser is a 1024-bin lower-bound table plus
// one or two threshold compares (exact: the bin table is derived from the thresholds), falling back to a binary
// search when the thresholds are too dense for that.
//
// The cube.  An 8-bit pixel has 2^24 possible values and the whole stage is a pure function of the value, so a plan evaluates that
// function ONCE for every value (color_cube_kernel: the pipeline above, 16.7 M evaluations -- one 4096 x 4096 image's worth of work) into
// a 64 MiB table of output pixels indexed by the input pixel, (blue << 16 | green << 8 | red) -> red | green << 8 | blue << 16.  Applying a
// plan is then ONE dword read per pixel and no arithmetic (color_cube_quad_kernel / color_cube_bytes_kernel); the table sits in HBM (a
// 4400th of it), the part of it an image touches -- a natural image occupies a small fraction of the colour cube -- in the L2 / Infinity
// Cache.  Results are those of the evaluating kernels by construction.  GS360_COLOR_CUBE=0 at plan creation keeps the per-pixel
// evaluation (A/B, or to save the 64 MiB).
#include <type_traits>

#include "gs360_kernels.h"

namespace gs360 {

namespace {

constexpr int kColorThreads = 256;
constexpr int kBins = 1024;
constexpr int kColorBlocks = 2048;   // persistent blocks of the dword-aligned path: 256 CUs x 8

struct __attribute__((packed, aligned(4))) F3 { float x, y, z; };

struct __attribute__((aligned(16))) CellEntry { float v[16]; };   // c00.xyz c10.xyz c01.xyz c11.xyz + 4 floats of padding

struct Cell {               // one channel's LUT cell: lower index, upper index, weight of the upper node
    int i0, i1;
    float f;
};

__device__ __forceinline__ Cell cell_of(float pos, int nmax) {
    // DF:651-653: idx0 = floor(pos); idx1 = min(idx0 + 1, max_index); frac = pos - idx0
    const float fl = floorf(pos);
    Cell c;
    c.i0 = (int)fl;
    c.i1 = min(c.i0 + 1, nmax);
    c.f = pos - fl;
    return c;
}

__device__ __forceinline__ float lerp_ref(float a, float b, float t) { return a + (b - a) * t; }   // DF:672-679

struct Lds {
    float pos[768];
    float thr[260];          // [0] unused, [1..255] thresholds, [256..] = +inf sentinels
    uint8_t bin[kBins];
};

// number of thresholds <= clip(x, 0, 1) among thr[1..255] (non-decreasing); NaN counts as 0
template <int FIX>
__device__ __forceinline__ int level_of(const Lds& S, float x) {
    const float xc = fminf(fmaxf(x, 0.0f), 1.0f);                       // fmaxf(NaN, 0) = 0
    if (FIX == 0) {          // general: binary search
        int lv = 0;
#pragma unroll
        for (int bit = 128; bit > 0; bit >>= 1) {
            const int cand = lv | bit;
            lv = (xc >= S.thr[cand]) ? cand : lv;
        }
        return lv;
    }
    int lv = S.bin[min((int)(xc * (float)kBins), kBins - 1)];           // thresholds <= the bin's lower edge
#pragma unroll
    for (int k = 0; k < FIX; ++k) lv += (xc >= S.thr[lv + 1]) ? 1 : 0;  // at most FIX thresholds lie inside a bin
    return lv;
}

struct Rgb { int r, g, b; };

// Pixel x of row y of an image side (strides are in bytes).
template <int C, typename T>
__device__ __forceinline__ T* pixel_at(const void* base, int64_t stride, int y, int x) {
    return (T*)((const char*)base + (int64_t)y * stride) + (int64_t)x * C;
}

// One pixel of T samples: read R/G/B through the memory index of the red channel (0 or 2), apply f(r, g, b) -> Rgb, keep alpha
// when C == 4, write back in memory order.
template <int C, typename T, typename F>
__device__ __forceinline__ void pixel_step(const ColorImage& I, int y, int x, F f) {
    const T* sp = pixel_at<C, const T>(I.src, I.src_stride, y, x);
    T* dp = pixel_at<C, T>(I.dst, I.dst_stride, y, x);
    const int iR = I.red_index, iB = 2 - I.red_index;
    const int alpha = (C == 4) ? sp[3] : 0;
    const Rgb q = f((int)sp[iR], (int)sp[1], (int)sp[iB]);
    dp[iR] = (T)q.r; dp[1] = (T)q.g; dp[iB] = (T)q.b;
    if (C == 4) dp[3] = (T)alpha;
}

// A group of pixels held in C dwords -- four 8-bit or two 16-bit pixels, BITS per sample, sample i at bit i * BITS of the group.
// The colour samples of pixel p as R, G, B ...
template <int C, int BITS>
__device__ __forceinline__ Rgb group_px(const uint32_t (&w)[C], int p, bool bgr) {
    auto get = [&](int i) { return (int)((w[i * BITS / 32] >> (i * BITS % 32)) & ((1u << BITS) - 1u)); };
    const int m0 = get(p * C), m2 = get(p * C + 2);
    return {bgr ? m2 : m0, get(p * C + 1), bgr ? m0 : m2};
}
// ... its output levels or-ed into an output group in memory order ...
template <int C, int BITS>
__device__ __forceinline__ void group_put(uint32_t (&o)[C], int p, bool bgr, const Rgb& q) {
    auto put = [&](int i, int v) { o[i * BITS / 32] |= (uint32_t)v << (i * BITS % 32); };
    put(p * C, bgr ? q.b : q.r);
    put(p * C + 1, q.g);
    put(p * C + 2, bgr ? q.r : q.b);
}
// ... and the output group to start from: every fourth sample (alpha, C == 4) kept, the colour samples zero.
template <int C, int BITS>
__device__ __forceinline__ void group_keep_alpha(const uint32_t (&w)[C], uint32_t (&o)[C]) {
#pragma unroll
    for (int i = 0; i < C; ++i) {
        uint32_t mask = 0u;
#pragma unroll
        for (int j = 0; j < 32 / BITS; ++j)
            if (C == 4 && (i * (32 / BITS) + j) % 4 == 3) mask |= ((1u << BITS) - 1u) << (j * BITS);
        o[i] = w[i] & mask;
    }
}

struct Taps {               // the four red-interpolated table entries around a pixel and its green/blue weights
    F3 c00, c10, c01, c11;
    float gf, bf;
};

// first half of the pipeline for one pixel: locate the cell and issue the table read (three aligned 16-byte loads of one entry)
__device__ __forceinline__ Taps color_fetch(const ColorLaunch& A, const Lds& S, int vr, int vg, int vb) {
    const int n = A.lut_size, nmax = n - 1;
    const Cell g = cell_of(S.pos[256 + vg], nmax);
    const Cell b = cell_of(S.pos[512 + vb], nmax);
    const char* base = (const char*)A.rtab;        // [blue cell][green cell][red level]; < 4 GiB: 32-bit byte offsets from a scalar base
    const float4* e = (const float4*)(base + (size_t)(((((uint32_t)(b.i0 * n + g.i0)) << 8) + (uint32_t)vr) << 6));
    const float4 q0 = e[0], q1 = e[1], q2 = e[2];
    Taps t;
    t.c00 = {q0.x, q0.y, q0.z};
    t.c10 = {q0.w, q1.x, q1.y};
    t.c01 = {q1.z, q1.w, q2.x};
    t.c11 = {q2.y, q2.z, q2.w};
    t.gf = g.f;
    t.bf = b.f;
    return t;
}

// second half: green stage, blue stage (DF:676-679), quantise
template <int FIX>
__device__ __forceinline__ Rgb color_finish(const Lds& S, const Taps& t) {
    Rgb q;
    q.r = level_of<FIX>(S, lerp_ref(lerp_ref(t.c00.x, t.c10.x, t.gf), lerp_ref(t.c01.x, t.c11.x, t.gf), t.bf));
    q.g = level_of<FIX>(S, lerp_ref(lerp_ref(t.c00.y, t.c10.y, t.gf), lerp_ref(t.c01.y, t.c11.y, t.gf), t.bf));
    q.b = level_of<FIX>(S, lerp_ref(lerp_ref(t.c00.z, t.c10.z, t.gf), lerp_ref(t.c01.z, t.c11.z, t.gf), t.bf));
    return q;
}

template <int FIX>
__device__ __forceinline__ Rgb color_px(const ColorLaunch& A, const Lds& S, int vr, int vg, int vb) {
    return color_finish<FIX>(S, color_fetch(A, S, vr, vg, vb));
}

// A.tables: 768 level positions (R,G,B x 256), 256 thresholds, then kBins/4 dwords of packed bin levels
__device__ __forceinline__ void load_tables(const ColorLaunch& A, Lds& S) {
    constexpr int kPer = (1024 + kBins / 4) / kColorThreads;               // 5 dwords per thread, all in flight at once
    static_assert((1024 + kBins / 4) % kColorThreads == 0, "table size");
    float v[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) v[j] = A.tables[j * kColorThreads + threadIdx.x];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int i = j * kColorThreads + threadIdx.x;
        if (i < 768) S.pos[i] = v[j];
        else if (i < 1024) S.thr[i - 768] = v[j];
        else ((float*)S.bin)[i - 1024] = v[j];
    }
    if (threadIdx.x < 4) S.thr[256 + threadIdx.x] = __builtin_inff();
    __syncthreads();
}

// Any alignment: one thread per pixel, byte loads and stores.
template <int C, int FIX>
__global__ __launch_bounds__(kColorThreads) void color_lut_bytes_kernel(ColorLaunch A) {
    __shared__ Lds S;
    load_tables(A, S);
    const int x = blockIdx.x * kColorThreads + threadIdx.x;
    if (x >= A.img.W) return;
    pixel_step<C, uint8_t>(A.img, blockIdx.y, x, [&](int r, int g, int b) { return color_px<FIX>(A, S, r, g, b); });
}

// Rows that start on a dword boundary: one thread per 4 pixels = C dwords in, C dwords out, so a wavefront moves
// 768 (C=3) or 1024 (C=4) contiguous bytes per row segment.  Blocks are persistent (the LDS tables are loaded once
// per block) and walk 1024-pixel row segments in row-major order.
constexpr int kColorWaves = 5;
template <int C, int FIX>
__global__ __launch_bounds__(kColorThreads) __attribute__((amdgpu_waves_per_eu(kColorWaves, kColorWaves))) void color_lut_quad_kernel(ColorLaunch A) {
    __shared__ Lds S;
    load_tables(A, S);
    const ColorImage& I = A.img;
    const bool bgr = I.red_index != 0;
    const int segs = (I.W + 4 * kColorThreads - 1) / (4 * kColorThreads);
    const int total = segs * I.H;
    // the image dwords of a thread's NEXT row segment are requested before the current one is worked on: of the chain image read ->
    // level tables (LDS) -> entry read -> blend -> quantiser tables (LDS) -> store, the first link then costs nothing
    auto seg_src = [&](int t, int& y, int& x) {
        y = t / segs;
        x = ((t - y * segs) * kColorThreads + threadIdx.x) * 4;
        return pixel_at<C, const uint8_t>(I.src, I.src_stride, y, x);
    };
    uint32_t wn[C];
#pragma unroll
    for (int i = 0; i < C; ++i) wn[i] = 0;
    {
        int y0, x0;
        const uint8_t* p0 = seg_src(blockIdx.x, y0, x0);
        if (blockIdx.x < (unsigned)total && x0 + 4 <= I.W) {
#pragma unroll
            for (int i = 0; i < C; ++i) wn[i] = ((const uint32_t*)p0)[i];
        }
    }
    for (int t = blockIdx.x; t < total; t += gridDim.x) {
        int y, x;
        seg_src(t, y, x);
        uint32_t w[C];
#pragma unroll
        for (int i = 0; i < C; ++i) w[i] = wn[i];
        {
            int yn, xn;
            const int tn = t + (int)gridDim.x;
            const uint8_t* pn = seg_src(tn, yn, xn);
            if (tn < total && xn + 4 <= I.W) {
#pragma unroll
                for (int i = 0; i < C; ++i) wn[i] = ((const uint32_t*)pn)[i];
            }
        }
        if (x >= I.W) continue;
        if (x + 4 <= I.W) {
            Taps taps[4];                          // all 16 table reads of the four pixels are in flight together
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const Rgb v = group_px<C, 8>(w, p, bgr);
                taps[p] = color_fetch(A, S, v.r, v.g, v.b);
            }
            __builtin_amdgcn_sched_barrier(0);     // keep the scheduler from sinking reads below the first blend
            uint32_t o[C];
            group_keep_alpha<C, 8>(w, o);
#pragma unroll
            for (int p = 0; p < 4; ++p) group_put<C, 8>(o, p, bgr, color_finish<FIX>(S, taps[p]));
            uint32_t* d32 = (uint32_t*)pixel_at<C, uint8_t>(I.dst, I.dst_stride, y, x);
#pragma unroll
            for (int i = 0; i < C; ++i) d32[i] = o[i];
        } else {
            for (int p = 0; x + p < I.W; ++p)
                pixel_step<C, uint8_t>(I, y, x + p, [&](int r, int g, int b) { return color_px<FIX>(A, S, r, g, b); });
        }
    }
}

// ---- the cube: every possible 8-bit pixel through the pipeline once, then one read per pixel ---------------------------------------
// A.cube: [blue][green][red] -> red | green << 8 | blue << 16
template <int FIX>
__global__ __launch_bounds__(kColorThreads) void color_cube_kernel(ColorLaunch A, uint32_t* cube) {
    __shared__ Lds S;
    load_tables(A, S);
    for (uint32_t i = blockIdx.x * kColorThreads + threadIdx.x; i < (1u << 24); i += gridDim.x * kColorThreads) {
        const Rgb q = color_px<FIX>(A, S, (int)(i & 255u), (int)((i >> 8) & 255u), (int)(i >> 16));
        cube[i] = (uint32_t)q.r | ((uint32_t)q.g << 8) | ((uint32_t)q.b << 16);
    }
}

template <int C>
__device__ __forceinline__ void cube_pixel_step(const ColorLaunch& A, int y, int x) {
    pixel_step<C, uint8_t>(A.img, y, x, [&](int r, int g, int b) {
        const uint32_t q = ((const uint32_t*)A.cube)[(uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16)];
        return Rgb{(int)q, (int)(q >> 8), (int)(q >> 16)};     // the store keeps the low byte of each
    });
}

// v_perm_b32 selectors (bytes 0-3 = the second operand, 0x0c = a zero byte): keep the three colour bytes of a pixel in memory order
// (red first) or swap the outer two (blue first); the swap is its own inverse, so the same selector turns a table entry back into
// memory order
__device__ __forceinline__ uint32_t cube_selector(int red) { return red != 0 ? 0x0c000102u : 0x0c020100u; }

template <int C>
__global__ __launch_bounds__(kColorThreads) void color_cube_bytes_kernel(ColorLaunch A) {
    const int x = blockIdx.x * kColorThreads + threadIdx.x;
    if (x < A.img.W) cube_pixel_step<C>(A, blockIdx.y, x);
}

// Rows that start on a dword boundary: a thread takes kCubeQuads groups of four pixels (C dwords in, four table reads, C dwords out each),
// the groups of a thread one wavefront-row (256 pixels x 4) apart so that every load and store instruction of a wavefront covers
// contiguous bytes; all table reads of a thread are in flight together.  (The unpacking is alignbit / perm by hand, not group_px.)
constexpr int kCubeQuads = 2;
template <int C>
__global__ __launch_bounds__(kColorThreads) void color_cube_quad_kernel(ColorLaunch A) {
    const ColorImage& I = A.img;
    const uint32_t* cube = (const uint32_t*)A.cube;
    const uint32_t sel = cube_selector(I.red_index);
    const int x0 = (blockIdx.x * kCubeQuads * kColorThreads + threadIdx.x) * 4;
    const int y = blockIdx.y;
    uint32_t w[kCubeQuads][C], q[kCubeQuads][4];
#pragma unroll
    for (int k = 0; k < kCubeQuads; ++k) {
        const int x = x0 + k * 4 * kColorThreads;
        if (x + 4 <= I.W) {
#pragma unroll
            for (int i = 0; i < C; ++i) w[k][i] = ((const uint32_t*)pixel_at<C, const uint8_t>(I.src, I.src_stride, y, x))[i];
        }
    }
#pragma unroll
    for (int k = 0; k < kCubeQuads; ++k) {
        const int x = x0 + k * 4 * kColorThreads;
        if (x + 4 <= I.W) {
            uint32_t px[4];
            if (C == 4) {
#pragma unroll
                for (int p = 0; p < 4; ++p) px[p] = w[k][p];
            } else {
                px[0] = w[k][0];
                px[1] = __builtin_amdgcn_alignbit(w[k][1], w[k][0], 24);
                px[2] = __builtin_amdgcn_alignbit(w[k][2], w[k][1], 16);
                px[3] = w[k][2] >> 8;
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) q[k][p] = cube[__builtin_amdgcn_perm(0u, px[p], sel)];
        }
    }
#pragma unroll
    for (int k = 0; k < kCubeQuads; ++k) {
        const int x = x0 + k * 4 * kColorThreads;
        if (x >= I.W) continue;
        if (x + 4 <= I.W) {
            uint32_t o[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) o[p] = __builtin_amdgcn_perm(0u, q[k][p], sel);
            uint32_t* d32 = (uint32_t*)pixel_at<C, uint8_t>(I.dst, I.dst_stride, y, x);
            if (C == 4) {
#pragma unroll
                for (int p = 0; p < 4; ++p) d32[p] = o[p] | (w[k][p] & 0xff000000u);
            } else {
                d32[0] = o[0] | (o[1] << 24);
                d32[1] = (o[1] >> 8) | (o[2] << 16);
                d32[2] = (o[2] >> 16) | (o[3] << 8);
            }
        } else {                                   // the last, partial group of a row
            for (int p = 0; x + p < I.W; ++p) cube_pixel_step<C>(A, y, x + p);
        }
    }
}

// Plan creation: the red stage of DF:672-675 for the four corners of every (blue cell, green cell) at every red level.  The upper
// neighbours are min(i + 1, n - 1) as in cell_of, so the last cell of an axis repeats its own node (its weight is then 0).
__global__ void color_rtab_kernel(const float* lut /* [b][g][r][3] */, const float* pos_r /* 256 */, CellEntry* rtab, int n) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * n * 256) return;
    const int level = idx & 255, cell = idx >> 8;         // cell = b0*n + g0
    const int b0 = cell / n, g0 = cell - b0 * n;
    const int b1 = min(b0 + 1, n - 1), g1 = min(g0 + 1, n - 1);
    const Cell r = cell_of(pos_r[level], n - 1);
    const int rows[4] = {b0 * n + g0, b0 * n + g1, b1 * n + g0, b1 * n + g1};    // c00, c10, c01, c11
    CellEntry o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float* lo = lut + ((size_t)rows[k] * n + r.i0) * 3;
        const float* hi = lut + ((size_t)rows[k] * n + r.i1) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) o.v[3 * k + c] = lerp_ref(lo[c], hi[c], r.f);
    }
    o.v[12] = o.v[13] = o.v[14] = o.v[15] = 0.0f;
    rtab[idx] = o;
}

// ---- 16-bit images (DF:603-618 handle uint16 like uint8, with 65535 levels) ------------------------------------------------
// With 65536 input levels per channel nothing is tabulated on the input side: float01 conversion, domain mapping, cell
// lookup and all three interpolation stages are evaluated per pixel with the reference's own float32 operations (IEEE
// division: the library is built with correctly rounded division).  Output side: `passthrough` is rint(clip(x) * 65535)
// in-kernel; the sRGB re-encode goes through NumPy's implementation-defined float32 power, so it arrives as sorted
// thresholds like the 8-bit path -- but in PIECES (the composite is only piecewise monotone at 16-bit resolution: Rec.709
// knee, sRGB toe): piece p covers clip(x) in [start[p], start[p+1]), level = base[p] + #(thresholds of p <= clip(x)).
constexpr int kBins16 = 65536;
struct __attribute__((aligned(16))) Bin16 {   // answers for x = b / 65536
    uint32_t kp;                               // piece that holds x << 28 | thresholds of that piece <= x (absolute index)
    float t[3];                                // the next three thresholds of the piece (+inf behind its end)
};

// how many of the sorted t[0..n) are <= x (upper bound)
__host__ __device__ inline int count_le(const float* t, int n, float x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (t[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The three output levels of a pixel.  A value's bin entry (one 16-byte read) counts the thresholds up to the bin's lower edge (<= the
// value: the scaling by 2^16 and the truncation are exact) and brings the next three along -- enough wherever the encode curve rises by
// less than three levels per 2^-16; past them the thresholds are counted one by one.  A bin that straddles a piece boundary (at most
// three do) takes the binary search instead.
__device__ __forceinline__ Rgb levels16_of(const Color16Launch& A, const float (&x)[3]) {
    float xc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) xc[c] = fminf(fmaxf(x[c], 0.0f), 1.0f);
    int q[3];
    if (A.n_pieces == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) q[c] = (int)__builtin_rintf(xc[c] * 65535.0f);
        return {q[0], q[1], q[2]};
    }
    const Bin16* bins = reinterpret_cast<const Bin16*>(A.bins);
    Bin16 e[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) e[c] = bins[min((int)(xc[c] * (float)kBins16), kBins16 - 1)];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int p = 0;
        if (A.n_pieces > 1 && xc[c] >= A.start[1]) p = 1;
        if (A.n_pieces > 2 && xc[c] >= A.start[2]) p = 2;
        if (A.n_pieces > 3 && xc[c] >= A.start[3]) p = 3;
        const int first = A.off[p], end = A.off[p + 1];
        int k;
        if ((int)(e[c].kp >> 28) == p) {
            k = (int)(e[c].kp & 0x0fffffffu);
            const int n3 = (e[c].t[0] <= xc[c] ? 1 : 0) + (e[c].t[1] <= xc[c] ? 1 : 0) + (e[c].t[2] <= xc[c] ? 1 : 0);   // sorted
            k += n3;
            if (n3 == 3)
                while (k < end && A.thr[k] <= xc[c]) ++k;
        } else {
            k = first + count_le(A.thr + first, end - first, xc[c]);
        }
        q[c] = A.base[p] + (k - first);
    }
    return {q[0], q[1], q[2]};
}

// one pixel: float01 conversion, domain mapping, cell lookup, the three interpolation stages in the reference's order, output levels
__device__ __forceinline__ Rgb color16_px(const Color16Launch& A, int vr, int vg, int vb) {
    const int n = A.lut_size, nmax = n - 1;
    const int v[3] = {vr, vg, vb};
    Cell c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float f01 = (float)v[k] / 65535.0f;                                        // DF:609-610
        const float coord = fminf(fmaxf((f01 - A.dmin[k]) / A.span[k], 0.0f), 1.0f);     // DF:647
        c[k] = cell_of(coord * (float)nmax, nmax);                                       // DF:648-653
    }
    // the eight corners as 12-byte nodes, all requested before the first blend
    const F3* T = reinterpret_cast<const F3*>(A.lut);
    auto at = [&](int bi, int gi, int ri) { return T[((uint32_t)bi * (uint32_t)n + (uint32_t)gi) * (uint32_t)n + (uint32_t)ri]; };
    const F3 n000 = at(c[2].i0, c[1].i0, c[0].i0), n001 = at(c[2].i0, c[1].i0, c[0].i1);
    const F3 n010 = at(c[2].i0, c[1].i1, c[0].i0), n011 = at(c[2].i0, c[1].i1, c[0].i1);
    const F3 n100 = at(c[2].i1, c[1].i0, c[0].i0), n101 = at(c[2].i1, c[1].i0, c[0].i1);
    const F3 n110 = at(c[2].i1, c[1].i1, c[0].i0), n111 = at(c[2].i1, c[1].i1, c[0].i1);
    auto stage3 = [&](float v000, float v001, float v010, float v011, float v100, float v101, float v110, float v111) {
        const float c00 = lerp_ref(v000, v001, c[0].f), c10 = lerp_ref(v010, v011, c[0].f);                         // DF:672-675
        const float c01 = lerp_ref(v100, v101, c[0].f), c11 = lerp_ref(v110, v111, c[0].f);
        return lerp_ref(lerp_ref(c00, c10, c[1].f), lerp_ref(c01, c11, c[1].f), c[2].f);                            // DF:676-679
    };
    const float xs[3] = {stage3(n000.x, n001.x, n010.x, n011.x, n100.x, n101.x, n110.x, n111.x),
                         stage3(n000.y, n001.y, n010.y, n011.y, n100.y, n101.y, n110.y, n111.y),
                         stage3(n000.z, n001.z, n010.z, n011.z, n100.z, n101.z, n110.z, n111.z)};
    return levels16_of(A, xs);
}

template <int C>
__device__ __forceinline__ void color16_pixel_step(const Color16Launch& A, int y, int x) {
    pixel_step<C, uint16_t>(A.img, y, x, [&](int r, int g, int b) { return color16_px(A, r, g, b); });
}

// Any alignment: one thread per pixel, 16-bit loads and stores.
template <int C>
__global__ __launch_bounds__(kColorThreads) void color_lut_u16_kernel(Color16Launch A) {
    const int x = blockIdx.x * kColorThreads + threadIdx.x;
    if (x < A.img.W) color16_pixel_step<C>(A, blockIdx.y, x);
}

// Rows that start on a dword boundary: one thread per two pixels = C dwords in, C dwords out (the texture path is what bounds this
// kernel -- 16-bit accesses cost an instruction each, like dwords)
template <int C>
__global__ __launch_bounds__(kColorThreads) void color_lut_u16_pair_kernel(Color16Launch A) {
    const ColorImage& I = A.img;
    const int x = (blockIdx.x * kColorThreads + threadIdx.x) * 2, y = blockIdx.y;
    if (x >= I.W) return;
    if (x + 2 > I.W) {                                  // the last pixel of an odd-width row
        color16_pixel_step<C>(A, y, x);
        return;
    }
    const bool bgr = I.red_index != 0;
    uint32_t w[C], o[C];
#pragma unroll
    for (int i = 0; i < C; ++i) w[i] = ((const uint32_t*)pixel_at<C, const uint16_t>(I.src, I.src_stride, y, x))[i];
    group_keep_alpha<C, 16>(w, o);                      // alpha: the high half of dwords 1 and 3
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const Rgb v = group_px<C, 16>(w, p, bgr);
        group_put<C, 16>(o, p, bgr, color16_px(A, v.r, v.g, v.b));
    }
#pragma unroll
    for (int i = 0; i < C; ++i) ((uint32_t*)pixel_at<C, uint16_t>(I.dst, I.dst_stride, y, x))[i] = o[i];
}

// ---- launches -----------------------------------------------------------------------------------------------------------------------
// the dword kernels need every row of both sides to start on a dword boundary
bool dword_aligned(const ColorImage& I) {
    return (((uintptr_t)I.src | (uintptr_t)I.dst | (uint64_t)I.src_stride | (uint64_t)I.dst_stride) & 3u) == 0;
}

// one block row per image row, `per_block` pixels of it per block
dim3 row_grid(const ColorImage& I, int per_block) { return dim3((unsigned)((I.W + per_block - 1) / per_block), (unsigned)I.H); }

// f(std::integral_constant) for the channel count (3 or 4) / the quantiser variant (color_build_bins: 1, 2 or 0) as a template argument
template <int N> using Int = std::integral_constant<int, N>;
template <typename F> void with_channels(int C, F f) { if (C == 3) f(Int<3>{}); else f(Int<4>{}); }
template <typename F> void with_fixups(int fixups, F f) { if (fixups == 1) f(Int<1>{}); else if (fixups == 2) f(Int<2>{}); else f(Int<0>{}); }

}  // namespace

size_t color_rtab_bytes(int lut_size) { return (size_t)lut_size * lut_size * 256 * sizeof(CellEntry); }
size_t color_tables_floats() { return 1024 + kBins / 4; }

// Host: derive the bin table from the thresholds; returns the number of in-bin fix-up compares needed (1 or 2),
// or 0 when some bin holds more than two thresholds (binary search variant).
int color_build_bins(const float* thr /* 256, [0] unused */, uint8_t* bins /* kBins */) {
    int worst = 0;
    for (int i = 0; i < kBins; ++i) {
        const float lo = (float)i / (float)kBins;                        // exact
        const float hi = (float)(i + 1) / (float)kBins;
        int below = 0, inside = 0;
        for (int k = 1; k < 256; ++k) {
            if (thr[k] <= lo) ++below;
            else if (i == kBins - 1 ? thr[k] <= 1.0f : thr[k] < hi) ++inside;
        }
        bins[i] = (uint8_t)below;
        if (inside > worst) worst = inside;
    }
    return worst <= 1 ? 1 : (worst == 2 ? 2 : 0);
}

size_t color16_bins_bytes() { return (size_t)kBins16 * sizeof(Bin16); }

// Host: bin b answers for x = b / 65536 -- the piece that holds x, how many of that piece's thresholds are <= x (as an absolute index
// into the concatenated threshold array; plan16 creation bounds it by 2^20) and the next three thresholds of the piece.
void color16_build_bins(int n_pieces, const float* start, const int32_t* off, const float* thr, void* bins_out) {
    Bin16* bins = static_cast<Bin16*>(bins_out);
    for (int b = 0; b < kBins16; ++b) {
        const float edge = (float)b / (float)kBins16;                    // exact
        int p = 0;
        for (int q = 1; q < n_pieces; ++q)
            if (edge >= start[q]) p = q;
        const int k = off[p] + count_le(thr + off[p], off[p + 1] - off[p], edge);   // the first threshold > edge
        bins[b].kp = ((uint32_t)p << 28) | (uint32_t)k;
        for (int j = 0; j < 3; ++j) bins[b].t[j] = k + j < off[p + 1] ? thr[k + j] : __builtin_inff();
    }
}

hipError_t build_color_rtab(const float* d_lut, const float* d_pos_r, void* d_rtab, int lut_size, hipStream_t s) {
    const int total = lut_size * lut_size * 256;
    hipLaunchKernelGGL(color_rtab_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d_lut, d_pos_r, (CellEntry*)d_rtab, lut_size);
    return hipGetLastError();
}

size_t color_cube_bytes() { return ((size_t)1 << 24) * sizeof(uint32_t); }

hipError_t build_color_cube(const ColorLaunch& L, void* d_cube, hipStream_t s) {
    with_fixups(L.fixups, [&](auto fix) {
        hipLaunchKernelGGL((color_cube_kernel<decltype(fix)::value>), dim3(kColorBlocks), dim3(kColorThreads), 0, s, L, (uint32_t*)d_cube);
    });
    return hipGetLastError();
}

hipError_t launch_color16(const Color16Launch& L, int C, hipStream_t s) {
    const bool aligned = dword_aligned(L.img);
    with_channels(C, [&](auto c) {
        constexpr int Cn = decltype(c)::value;
        if (aligned) hipLaunchKernelGGL((color_lut_u16_pair_kernel<Cn>), row_grid(L.img, 2 * kColorThreads), dim3(kColorThreads), 0, s, L);
        else hipLaunchKernelGGL((color_lut_u16_kernel<Cn>), row_grid(L.img, kColorThreads), dim3(kColorThreads), 0, s, L);
    });
    return hipGetLastError();
}

hipError_t launch_color(const ColorLaunch& L, int C, hipStream_t s) {
    const ColorImage& I = L.img;
    const bool aligned = dword_aligned(I);
    const dim3 block(kColorThreads);
    with_channels(C, [&](auto c) {
        constexpr int Cn = decltype(c)::value;
        if (L.cube) {
            if (aligned) hipLaunchKernelGGL((color_cube_quad_kernel<Cn>), row_grid(I, 4 * kCubeQuads * kColorThreads), block, 0, s, L);
            else hipLaunchKernelGGL((color_cube_bytes_kernel<Cn>), row_grid(I, kColorThreads), block, 0, s, L);
            return;
        }
        with_fixups(L.fixups, [&](auto fix) {
            constexpr int FIX = decltype(fix)::value;
            if (aligned) {                       // persistent blocks over the 1024-pixel row segments
                const long total = (long)row_grid(I, 4 * kColorThreads).x * I.H;
                hipLaunchKernelGGL((color_lut_quad_kernel<Cn, FIX>), dim3((unsigned)(total < kColorBlocks ? total : kColorBlocks)), block, 0, s, L);
            } else {
                hipLaunchKernelGGL((color_lut_bytes_kernel<Cn, FIX>), row_grid(I, kColorThreads), block, 0, s, L);
            }
        });
    });
    return hipGetLastError();
}

}  // namespace gs360
