// gs360_frameflow.hip -- the FrameSelector's optical-flow motion on the GPU (include/gs360.h, "frame optical flow").
//
// Reference: _load_flow_gray / _compute_pair_flow_magnitude, cli_tools/gs360_FrameSelector.py:1245-1337, with FLOW_METHOD
// "lucas_kanade": cv2.goodFeaturesToTrack (1000 corners, quality 0.01, distance 5, block 7) on the previous frame and
// cv2.calcOpticalFlowPyrLK (window 15, 2 levels, 10 iterations / eps 0.03).  FS-FLOW v1 restates OpenCV
// 4.x's arithmetic with exact integers wherever OpenCV's values are integers; every float32 step below follows it op by op.
//
// Per frame (fl_small, fl_pyr, fl_pad, fl_eig, fl_cand, the bitonic sort, fl_select), once per frame of a call:
//   fl_small    crop + gray + INTER_AREA (integer-factor block sums or the general float32 tables) into the level-0 plane, and
//               the INTER_NEAREST circle mask
//   fl_pyr      pyrDown of level l-1 into level l's plane
//   fl_pad      the 15-pixel reflect-101 border of each level's plane and its Scharr derivatives (zero border)
//   fl_eig      cornerMinEigenVal: Sobel from the padded level 0, exact 7 x 7 sums, float32 from a, b, c; the masked maximum
//   fl_cand     threshold, 3 x 3 dilate, candidate keys (value bits << 32 | address)
//   sort        descending bitonic sort of the keys: greaterThanPtr's order (value, then the later address)
//   fl_select   the greedy minDistance grid, one wavefront per frame, 64 candidates at a time
// Per pair (fl_lk, fl_pair): one wavefront per corner runs the pyramid LK; one wavefront per pair sums the magnitudes in point
// order.  Frame state lives in the context's per-slot scratch (resident slots, so a frame in two pairs is computed once); the
// only atomics are integer counts and an integer maximum.
#include "gs360_framepx.h"

namespace gs360 {

namespace {

constexpr int kT = 256;
constexpr int kPad = 15;              // winSize: the pyramid border and the LK window
constexpr int kWin = 15;
constexpr int kGridCells = 64 * 64;   // minDistance grid of a <= 320 x 320 image (cell 5)

__device__ __forceinline__ int bint(int p, int n) {   // cv::borderInterpolate, BORDER_REFLECT_101, any distance
    if (n == 1) return 0;
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * n - 2 - p;
    return p;
}

__device__ __forceinline__ uint8_t sat_u8(float v) {   // saturate_cast<uchar>(float): round half to even, clamp
    const int i = (int)__builtin_rintf(v);
    return (uint8_t)min(max(i, 0), 255);
}

__device__ __forceinline__ uint8_t* plane(const FlLaunch& L, int slot, int lev) { return L.state + (size_t)slot * L.state_bytes + L.img_off[lev]; }
__device__ __forceinline__ short2* deriv(const FlLaunch& L, int slot, int lev) {
    return (short2*)(L.state + (size_t)slot * L.state_bytes + L.der_off[lev]);
}
__device__ __forceinline__ uint8_t* work(const FlLaunch& L, int b) { return L.work + (size_t)b * L.work_bytes; }
__device__ __forceinline__ FlCounters* counters(const FlLaunch& L, int b) { return (FlCounters*)(work(L, b) + L.cnt_off); }
__device__ __forceinline__ unsigned ordered(float v) {   // float -> unsigned with the same order (for an integer maximum)
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unordered(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

// 1. crop, gray, INTER_AREA to sw x sh into level 0's plane; the circle at INTER_NEAREST's sample.  T: the sample type; a uint16_t
// frame is read through its 8-bit view (FS-DEPTH16 v1), so everything after this kernel is FS-FLOW v1 unchanged.
template <int C, typename T>
__global__ void __launch_bounds__(kT) fl_small(const FlLaunch L) {
    constexpr int kPx = C * (int)sizeof(T);                 // bytes per pixel
    const int dx = blockIdx.x * kT + threadIdx.x, dy = blockIdx.y, b = blockIdx.z;
    const bool in = dx < L.sw;
    int inmask = 0;
    if (in) {
        const uint8_t* crop = L.src[b] + (int64_t)L.cy0 * L.stride + (int64_t)L.cx0 * kPx;
        int v;
        if (L.mode == 0) {                 // no resize: the crop itself
            v = gray8_of<C, T>(crop + (int64_t)dy * L.stride + dx * kPx, L.red);
        } else if (L.mode == 1) {          // integer factors kx x ky: int block sum * float32(1 / area)
            int s = 0;
            for (int yy = 0; yy < L.ky; ++yy) {
                const uint8_t* r = crop + (int64_t)(dy * L.ky + yy) * L.stride + (int64_t)dx * L.kx * kPx;
                for (int xx = 0; xx < L.kx; ++xx) s += gray8_of<C, T>(r + xx * kPx, L.red);
            }
            v = sat_u8((float)s * (1.0f / (float)(L.kx * L.ky)));
        } else {                           // general float32 tables, ResizeArea_Invoker's order
            const AreaSpan ax = area_span(dx, L.cw, L.scale_x), ay = area_span(dy, L.ch, L.scale_y);
            float sum = 0.0f;
            if (ay.has_head) sum += ay.head * area_row<C, T, true>(crop + (int64_t)(ay.i1 - 1) * L.stride, ax, L.red);
            for (int sy = ay.i1; sy < ay.i2; ++sy) sum += ay.mid * area_row<C, T, true>(crop + (int64_t)sy * L.stride, ax, L.red);
            if (ay.has_tail) sum += ay.tail * area_row<C, T, true>(crop + (int64_t)ay.i2 * L.stride, ax, L.red);
            v = sat_u8(sum);
        }
        plane(L, L.slot[b], 0)[(int64_t)(dy + kPad) * L.pitch[0] + dx + kPad] = (uint8_t)v;
        if (L.circle) {   // INTER_NEAREST of the full-frame circle, cropped
            const int nx = L.cx0 + nearest_index(dx, L.scale_x, L.cw);
            const int ny = L.cy0 + nearest_index(dy, L.scale_y, L.ch);
            const int64_t ex = 2 * (int64_t)nx - (L.W - 1), ey = 2 * (int64_t)ny - (L.H - 1);
            const int64_t mwh = min(L.W, L.H);       // circle_r4 written out: the helper changes this kernel's schedule
            inmask = ex * ex + ey * ey <= max((int64_t)4, mwh * mwh);
        }
        work(L, b)[L.mask_off + (int64_t)dy * L.sw + dx] = (uint8_t)inmask;
    }
    const unsigned long long bal = __ballot(inmask);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&counters(L, b)->n_mask, (int)__popcll(bal));
}

// 2. pyrDown: 5 x 5 [1 4 6 4 1]^2 / 256, (+128) >> 8, reflect-101 on the source level
__global__ void __launch_bounds__(kT) fl_pyr(const FlLaunch L, int lev) {
    const int dx = blockIdx.x * kT + threadIdx.x, dy = blockIdx.y, b = blockIdx.z;
    const int w = L.lw[lev], sw = L.lw[lev - 1], sh = L.lh[lev - 1];
    if (dx >= w) return;
    const uint8_t* s = plane(L, L.slot[b], lev - 1) + (int64_t)kPad * L.pitch[lev - 1] + kPad;
    const int wt[5] = {1, 4, 6, 4, 1};
    int xs[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) xs[k] = bint(2 * dx + k - 2, sw);
    int acc = 0;
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        const uint8_t* row = s + (int64_t)bint(2 * dy + r - 2, sh) * L.pitch[lev - 1];
        int rs = 0;
#pragma unroll
        for (int k = 0; k < 5; ++k) rs += wt[k] * row[xs[k]];
        acc += wt[r] * rs;
    }
    plane(L, L.slot[b], lev)[(int64_t)(dy + kPad) * L.pitch[lev] + dx + kPad] = (uint8_t)min((acc + 128) >> 8, 255);
}

// 3. the reflect-101 border of a level's plane (interior untouched), then (fl_deriv) calcSharrDeriv with a zero border
__global__ void __launch_bounds__(kT) fl_pad(const FlLaunch L, int lev) {
    const int px = blockIdx.x * kT + threadIdx.x, py = blockIdx.y, b = blockIdx.z;
    const int w = L.lw[lev], h = L.lh[lev], P = L.pitch[lev];
    if (px >= w + 2 * kPad) return;
    const int x = px - kPad, y = py - kPad;
    if (x >= 0 && x < w && y >= 0 && y < h) return;
    uint8_t* p = plane(L, L.slot[b], lev);
    p[(int64_t)py * P + px] = p[(int64_t)(bint(y, h) + kPad) * P + bint(x, w) + kPad];
}

__global__ void __launch_bounds__(kT) fl_deriv(const FlLaunch L, int lev) {
    const int px = blockIdx.x * kT + threadIdx.x, py = blockIdx.y, b = blockIdx.z;
    const int w = L.lw[lev], h = L.lh[lev], P = L.pitch[lev];
    if (px >= w + 2 * kPad) return;
    const int x = px - kPad, y = py - kPad;
    short2 d = make_short2(0, 0);
    if (x >= 0 && x < w && y >= 0 && y < h) {   // the padded plane holds calcSharrDeriv's one-step reflect-101 neighbours
        const uint8_t* p = plane(L, L.slot[b], lev) + (int64_t)py * P + px;
        auto t0 = [&](int o) { return (p[o - P] + p[o + P]) * 3 + p[o] * 10; };
        auto t1 = [&](int o) { return p[o + P] - p[o - P]; };
        d.x = (short)(t0(1) - t0(-1));
        d.y = (short)((t1(1) + t1(-1)) * 3 + t1(0) * 10);
    }
    deriv(L, L.slot[b], lev)[(int64_t)py * P + px] = d;
}

// 4. cornerMinEigenVal (block 7, Sobel 3): Sobel as ints from the padded level 0, 7 x 7 int sums with reflect-101, then float32
__global__ void __launch_bounds__(kT) fl_sobel(const FlLaunch L) {
    const int x = blockIdx.x * kT + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= L.sw) return;
    const int P = L.pitch[0];
    const uint8_t* p = plane(L, L.slot[b], 0) + (int64_t)(y + kPad) * P + x + kPad;
    const int gx = (p[1 - P] + 2 * p[1] + p[1 + P]) - (p[-1 - P] + 2 * p[-1] + p[-1 + P]);
    const int gy = (p[P - 1] + 2 * p[P] + p[P + 1]) - (p[-P - 1] + 2 * p[-P] + p[-P + 1]);
    ((short2*)(work(L, b) + L.sob_off))[(int64_t)y * L.sw + x] = make_short2((short)gx, (short)gy);
}

__global__ void __launch_bounds__(kT) fl_eig(const FlLaunch L) {
    const int x = blockIdx.x * kT + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    const int w = L.sw, h = L.sh;
    const FlCounters* cn = counters(L, b);
    const bool use_mask = L.circle && cn->n_mask > 0;
    unsigned key = 0;
    if (x < w) {
        const short2* sob = (const short2*)(work(L, b) + L.sob_off);
        int xs[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) xs[k] = bint(x + k - 3, w);
        int sxx = 0, sxy = 0, syy = 0;   // <= 49 * 1020^2 < 2^31
        for (int r = 0; r < 7; ++r) {
            const short2* row = sob + (int64_t)bint(y + r - 3, h) * w;
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                const short2 g = row[xs[k]];
                sxx += g.x * g.x; sxy += g.x * g.y; syy += g.y * g.y;
            }
        }
        const double K = 1.0 / 50979600.0;   // (1 / (4 * 7 * 255))^2
        const float a = (float)((double)sxx * (K * 0.5)), bb = (float)((double)sxy * K), c = (float)((double)syy * (K * 0.5));
        const float e = (a + c) - sqrtf((a - c) * (a - c) + bb * bb);
        ((float*)(work(L, b) + L.eig_off))[(int64_t)y * w + x] = e;
        if (!use_mask || work(L, b)[L.mask_off + (int64_t)y * w + x]) key = ordered(e);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) key = max(key, (unsigned)__shfl_xor((int)key, o, 64));
    if ((threadIdx.x & 63) == 0 && key) atomicMax(&counters(L, b)->max_key, key);
}

// 5. THRESH_TOZERO at float32(maxVal * 0.01), 3 x 3 dilate, candidates 1 <= x <= w-2, 1 <= y <= h-2 inside the mask
__global__ void __launch_bounds__(kT) fl_cand(const FlLaunch L) {
    const int x = blockIdx.x * kT + threadIdx.x + 1, y = blockIdx.y + 1, b = blockIdx.z;
    const int w = L.sw;
    if (x > w - 2) return;
    FlCounters* cn = counters(L, b);
    const float thr = (float)((double)unordered(cn->max_key) * 0.01);
    const float* eig = (const float*)(work(L, b) + L.eig_off);
    auto t = [&](int xx, int yy) { const float v = eig[(int64_t)yy * w + xx]; return v > thr ? v : 0.0f; };
    const float v = t(x, y);
    if (v == 0.0f) return;
    float d = v;
    for (int oy = -1; oy <= 1; ++oy)
        for (int ox = -1; ox <= 1; ++ox) d = fmaxf(d, t(x + ox, y + oy));
    if (v != d) return;
    if (L.circle && cn->n_mask > 0 && !work(L, b)[L.mask_off + (int64_t)y * w + x]) return;
    const int pos = atomicAdd(&cn->n_cand, 1);
    ((uint64_t*)(work(L, b) + L.key_off))[pos] = ((uint64_t)__float_as_uint(v) << 32) | (uint32_t)(y * w + x);
}

// 6. descending bitonic sort of each frame's keys (zero beyond the count); stages above the frame's next power of two are skipped
__device__ __forceinline__ int frame_n2(const FlLaunch& L, int b) {
    int n = counters(L, b)->n_cand, p = 1;
    while (p < n) p <<= 1;
    return p;
}

constexpr int kSortLocal = 2048;   // keys one 1024-thread workgroup sorts / merges in LDS

__global__ void __launch_bounds__(1024) fl_sort_local(const FlLaunch L, int k_first) {
    // k_first == 0: every stage k <= kSortLocal of this chunk; else the j < kSortLocal steps of stage k_first
    __shared__ uint64_t s[kSortLocal];
    const int b = blockIdx.y;
    const int base = blockIdx.x * kSortLocal;
    const int n2 = frame_n2(L, b);
    if (base >= n2 || (k_first && k_first > n2) || n2 < 2) return;
    uint64_t* keys = (uint64_t*)(work(L, b) + L.key_off) + base;
    const int t = threadIdx.x;
    s[t] = keys[t];
    s[t + 1024] = keys[t + 1024];
    __syncthreads();
    const int k_lo = k_first ? k_first : 2, k_hi = k_first ? k_first : min(kSortLocal, n2);
    for (int k = k_lo; k <= k_hi; k <<= 1) {
        for (int j = min(k, kSortLocal) >> 1; j > 0; j >>= 1) {
            const int i = 2 * t - (t & (j - 1));       // the lower index of this thread's pair
            const int l = i + j;
            const bool desc = ((base + i) & k) == 0;
            const uint64_t a = s[i], c = s[l];
            if (desc ? a < c : a > c) { s[i] = c; s[l] = a; }
            __syncthreads();
        }
    }
    keys[t] = s[t];
    keys[t + 1024] = s[t + 1024];
}

__global__ void __launch_bounds__(kT) fl_sort_global(const FlLaunch L, int k, int j) {
    const int b = blockIdx.y;
    const int t = blockIdx.x * kT + threadIdx.x;   // pair index
    if (k > frame_n2(L, b)) return;
    const int i = 2 * t - (t & (j - 1)), l = i + j;
    if (l >= L.key_cap) return;
    uint64_t* keys = (uint64_t*)(work(L, b) + L.key_off);
    const bool desc = (i & k) == 0;
    const uint64_t a = keys[i], c = keys[l];
    if (desc ? a < c : a > c) { keys[i] = c; keys[l] = a; }
}

// 7. greedy minDistance selection: one wavefront per frame, 64 sorted candidates at a time
__global__ void __launch_bounds__(64) fl_select(const FlLaunch L) {
    __shared__ int cnt[kGridCells];
    __shared__ uint32_t pts[kGridCells][2];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int w = L.sw, h = L.sh;
    const int gw = (w + 4) / 5, gh = (h + 4) / 5;
    for (int i = lane; i < gw * gh; i += 64) cnt[i] = 0;
    __syncthreads();
    const int n = counters(L, b)->n_cand;
    const uint64_t* keys = (const uint64_t*)(work(L, b) + L.key_off);
    float2* corners = (float2*)(L.state + (size_t)L.slot[b] * L.state_bytes + L.corner_off);
    int acc = 0;
    for (int base = 0; base < n && acc < GS360_FLOW_MAX_CORNERS; base += 64) {
        const int i = base + lane;
        int x = 0, y = 0, cx = 0, cy = 0;
        bool good = i < n;
        if (good) {
            const uint32_t idx = (uint32_t)keys[i];
            y = (int)(idx / (uint32_t)w);
            x = (int)(idx - (uint32_t)y * w);
            cx = x / 5; cy = y / 5;
            for (int yy = max(0, cy - 1); yy <= min(gh - 1, cy + 1); ++yy)
                for (int xx = max(0, cx - 1); xx <= min(gw - 1, cx + 1); ++xx) {
                    const int c = yy * gw + xx;
                    for (int m = 0; m < cnt[c]; ++m) {
                        const int px = (int)(pts[c][m] & 0xffff), py = (int)(pts[c][m] >> 16);
                        if ((x - px) * (x - px) + (y - py) * (y - py) < 25) good = false;
                    }
                }
        }
        // resolve the batch in candidate order: each accepted lane removes the later lanes within distance 5
        unsigned long long todo = __ballot(good);
        while (todo) {
            const int k = __ffsll((long long)todo) - 1;
            const int xk = __shfl(x, k, 64), yk = __shfl(y, k, 64);
            if (acc == GS360_FLOW_MAX_CORNERS) break;
            if (lane == k) {
                const int c = cy * gw + cx;
                if (cnt[c] < 2) pts[c][cnt[c]] = (uint32_t)x | ((uint32_t)y << 16);   // two points per 5 x 5 cell at most
                cnt[c] = cnt[c] + 1;
                corners[acc] = make_float2((float)x, (float)y);
            }
            ++acc;
            if (lane > k && good && (x - xk) * (x - xk) + (y - yk) * (y - yk) < 25) good = false;
            todo = __ballot(good) & ~((2ull << k) - 1ull);
        }
        __syncthreads();
    }
    if (lane == 0) *(int*)(L.state + (size_t)L.slot[b] * L.state_bytes + L.ncorner_off) = acc;
}

// 8. pyramid Lucas-Kanade: one wavefront per corner; the 15 x 15 window as lane + 64 k, k < 4 (225 pixels)
__device__ __forceinline__ int descale(int v, int n) { return (v + (1 << (n - 1))) >> n; }

struct Wts { int w00, w01, w10, w11; };
__device__ __forceinline__ Wts weights(float a, float b) {
    Wts w;
    w.w00 = (int)__builtin_rintf(((1.f - a) * (1.f - b)) * 16384.f);
    w.w01 = (int)__builtin_rintf((a * (1.f - b)) * 16384.f);
    w.w10 = (int)__builtin_rintf(((1.f - a) * b) * 16384.f);
    w.w11 = 16384 - w.w00 - w.w01 - w.w10;
    return w;
}

__global__ void __launch_bounds__(kT) fl_lk(const FlLaunch L, const FlPairs Q) {
    const int pair = blockIdx.y, lane = threadIdx.x & 63;
    const int pt = blockIdx.x * (kT / 64) + (threadIdx.x >> 6);
    const int sp = Q.prev[pair], sc = Q.curr[pair];
    const uint8_t* stp = L.state + (size_t)sp * L.state_bytes;
    const int n = *(const int*)(stp + L.ncorner_off);
    if (pt >= n) return;
    const float2 p0 = ((const float2*)(stp + L.corner_off))[pt];
    const float hw = 7.0f, FS = 1.0f / (1 << 20);
    bool status = true;
    float nx = 0.f, ny = 0.f;   // nextPts[ptidx]
    for (int lev = L.levels - 1; lev >= 0; --lev) {
        const int cols = L.lw[lev], rows = L.lh[lev], P = L.pitch[lev];
        const uint8_t* I = plane(L, sp, lev);
        const uint8_t* J = plane(L, sc, lev);
        const short2* D = deriv(L, sp, lev);
        const float sc_l = 1.0f / (float)(1 << lev);
        const float prx = p0.x * sc_l - hw, pry = p0.y * sc_l - hw;
        float gx, gy;
        if (lev == L.levels - 1) { gx = p0.x * sc_l; gy = p0.y * sc_l; } else { gx = nx * 2.f; gy = ny * 2.f; }
        nx = gx; ny = gy;
        const int ipx = (int)floorf(prx), ipy = (int)floorf(pry);
        if (ipx < -kWin || ipx >= cols || ipy < -kWin || ipy >= rows) {
            if (lev == 0) status = false;
            continue;
        }
        Wts w = weights(prx - (float)ipx, pry - (float)ipy);
        int iv[4], ixv[4], iyv[4];
        long long a11 = 0, a12 = 0, a22 = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int q = lane + 64 * k;
            iv[k] = ixv[k] = iyv[k] = 0;
            if (q < kWin * kWin) {
                const int wy = q / kWin, wx = q - wy * kWin;
                const int64_t o = (int64_t)(ipy + wy + kPad) * P + ipx + wx + kPad;
                iv[k] = descale(I[o] * w.w00 + I[o + 1] * w.w01 + I[o + P] * w.w10 + I[o + P + 1] * w.w11, 9);
                const short2 d00 = D[o], d01 = D[o + 1], d10 = D[o + P], d11 = D[o + P + 1];
                ixv[k] = descale(d00.x * w.w00 + d01.x * w.w01 + d10.x * w.w10 + d11.x * w.w11, 14);
                iyv[k] = descale(d00.y * w.w00 + d01.y * w.w01 + d10.y * w.w10 + d11.y * w.w11, 14);
                a11 += (long long)ixv[k] * ixv[k];
                a12 += (long long)ixv[k] * iyv[k];
                a22 += (long long)iyv[k] * iyv[k];
            }
        }
        const float A11 = (float)(double)wave_sum(a11) * FS, A12 = (float)(double)wave_sum(a12) * FS, A22 = (float)(double)wave_sum(a22) * FS;
        float Dt = A11 * A22 - A12 * A12;
        const float minEig = ((A22 + A11) - sqrtf((A11 - A22) * (A11 - A22) + (4.f * A12) * A12)) / (float)(2 * kWin * kWin);
        if (minEig < 1e-4f || Dt < 1.1920929e-07f) {
            if (lev == 0) status = false;
            continue;
        }
        Dt = 1.f / Dt;
        float cx = nx - hw, cy = ny - hw;
        float pdx = 0.f, pdy = 0.f;
        for (int j = 0; j < 10; ++j) {
            const int inx = (int)floorf(cx), iny = (int)floorf(cy);
            if (inx < -kWin || inx >= cols || iny < -kWin || iny >= rows) {
                if (lev == 0) status = false;
                break;
            }
            w = weights(cx - (float)inx, cy - (float)iny);
            long long b1 = 0, b2 = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int q = lane + 64 * k;
                if (q < kWin * kWin) {
                    const int wy = q / kWin, wx = q - wy * kWin;
                    const int64_t o = (int64_t)(iny + wy + kPad) * P + inx + wx + kPad;
                    const int diff = descale(J[o] * w.w00 + J[o + 1] * w.w01 + J[o + P] * w.w10 + J[o + P + 1] * w.w11, 9) - iv[k];
                    b1 += (long long)diff * ixv[k];
                    b2 += (long long)diff * iyv[k];
                }
            }
            const float B1 = (float)(double)wave_sum(b1) * FS, B2 = (float)(double)wave_sum(b2) * FS;
            const float dx = (A12 * B2 - A22 * B1) * Dt, dy = (A12 * B1 - A11 * B2) * Dt;
            cx += dx; cy += dy;
            nx = cx + hw; ny = cy + hw;
            if ((double)dx * dx + (double)dy * dy <= 0.03 * 0.03) break;
            if (j > 0 && fabs((double)(dx + pdx)) < 0.01 && fabs((double)(dy + pdy)) < 0.01) {
                nx -= dx * 0.5f; ny -= dy * 0.5f;
                break;
            }
            pdx = dx; pdy = dy;
        }
    }
    if (lane == 0) {
        gs360_flow_point r;
        r.x0 = p0.x; r.y0 = p0.y; r.x1 = nx; r.y1 = ny; r.status = status ? 1 : 0; r.pad = 0;
        Q.points[(size_t)pair * GS360_FLOW_MAX_CORNERS + pt] = r;
    }
}

// 9. the pair record: sqrt(dx^2 + dy^2) in float32, summed in double in point order
__global__ void __launch_bounds__(64) fl_pair(const FlLaunch L, const FlPairs Q) {
    const int pair = blockIdx.x;
    if (threadIdx.x != 0) return;
    const int n = *(const int*)(L.state + (size_t)Q.prev[pair] * L.state_bytes + L.ncorner_off);
    const gs360_flow_point* p = Q.points + (size_t)pair * GS360_FLOW_MAX_CORNERS;
    gs360_flow_point* user = Q.user_points ? Q.user_points + (size_t)Q.out_index[pair] * GS360_FLOW_MAX_CORNERS : nullptr;
    long long nt = 0;
    double s = 0.0;
    for (int i = 0; i < n; ++i) {
        const gs360_flow_point r = p[i];
        if (user) user[i] = r;
        if (r.status) {
            const float dx = r.x1 - r.x0, dy = r.y1 - r.y0;
            s += (double)sqrtf(dx * dx + dy * dy);
            ++nt;
        }
    }
    gs360_frame_flow rec;
    rec.n_corners = n; rec.n_tracked = nt; rec.sum_mag = s;
    Q.out[Q.out_index[pair]] = rec;
}

inline dim3 g2(int w, int h, int nf) { return dim3((unsigned)((w + kT - 1) / kT), (unsigned)h, (unsigned)nf); }

template <int C, typename T>
hipError_t launch_frames_c(const FlLaunch& L, hipStream_t s) {
    const int nf = L.n_frames;
    hipLaunchKernelGGL((fl_small<C, T>), g2(L.sw, L.sh, nf), dim3(kT), 0, s, L);
    for (int lev = 0; lev < L.levels; ++lev) {
        if (lev) hipLaunchKernelGGL(fl_pyr, g2(L.lw[lev], L.lh[lev], nf), dim3(kT), 0, s, L, lev);
        hipLaunchKernelGGL(fl_pad, g2(L.lw[lev] + 2 * kPad, L.lh[lev] + 2 * kPad, nf), dim3(kT), 0, s, L, lev);
        hipLaunchKernelGGL(fl_deriv, g2(L.lw[lev] + 2 * kPad, L.lh[lev] + 2 * kPad, nf), dim3(kT), 0, s, L, lev);
    }
    hipLaunchKernelGGL(fl_sobel, g2(L.sw, L.sh, nf), dim3(kT), 0, s, L);
    hipLaunchKernelGGL(fl_eig, g2(L.sw, L.sh, nf), dim3(kT), 0, s, L);
    if (L.sw >= 3 && L.sh >= 3) hipLaunchKernelGGL(fl_cand, g2(L.sw - 2, L.sh - 2, nf), dim3(kT), 0, s, L);
    const int N = L.key_cap;   // a power of two >= kSortLocal
    hipLaunchKernelGGL(fl_sort_local, dim3((unsigned)(N / kSortLocal), (unsigned)nf), dim3(1024), 0, s, L, 0);
    for (int k = 2 * kSortLocal; k <= N; k <<= 1) {
        for (int j = k >> 1; j >= kSortLocal; j >>= 1)
            hipLaunchKernelGGL(fl_sort_global, dim3((unsigned)(N / 2 / kT), (unsigned)nf), dim3(kT), 0, s, L, k, j);
        hipLaunchKernelGGL(fl_sort_local, dim3((unsigned)(N / kSortLocal), (unsigned)nf), dim3(1024), 0, s, L, k);
    }
    hipLaunchKernelGGL(fl_select, dim3((unsigned)nf), dim3(64), 0, s, L);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_frames_t(const FlLaunch& L, hipStream_t s) {
    switch (L.C) {
        case 1: return launch_frames_c<1, T>(L, s);
        case 3: return launch_frames_c<3, T>(L, s);
        case 4: return launch_frames_c<4, T>(L, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_frame_flow_frames(const FlLaunch& L, hipStream_t s) {
    return L.depth == 16 ? launch_frames_t<uint16_t>(L, s) : launch_frames_t<uint8_t>(L, s);
}

hipError_t launch_frame_flow_pairs(const FlLaunch& L, const FlPairs& Q, hipStream_t s) {
    hipLaunchKernelGGL(fl_lk, dim3((unsigned)(GS360_FLOW_MAX_CORNERS + kT / 64 - 1) / (kT / 64), (unsigned)Q.n_pairs), dim3(kT), 0, s, L, Q);
    hipLaunchKernelGGL(fl_pair, dim3((unsigned)Q.n_pairs), dim3(64), 0, s, L, Q);
    return hipGetLastError();
}

}  // namespace gs360
