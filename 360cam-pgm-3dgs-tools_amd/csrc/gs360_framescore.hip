// gs360_framescore.hip -- the FrameSelector's per-pixel scoring pass on the GPU (include/gs360.h, "frame sharpness statistics").
//
// Reference: score_one_file, cli_tools/gs360_FrameSelector.py:902-1044 with lapvar32 / tenengrad32 (FS:720-739) and the INTER_AREA
// input of fft_energy_fast (FS:742-786).  FS-SPEC v1 restates all of it for 8-bit sources as integer arithmetic: the gray
// values, the Laplacian and the Sobel responses are small integers, so their sums are exact and this kernel reproduces the
// double accumulators of cv2.meanStdDev / cv2.mean bit for bit, whatever the order in which workgroups finish.
//
// FS-DEPTH16 v1 is the same for 16-bit sources: the kernels take the sample type T, the statistics run on the 16-bit
// gray (sums in units of 1/257 gray level), the edge pass on the samples' high bytes.
//
// fs_strip_kernel<C, T, false>, the statistics pass: one 256-thread workgroup per strip of kFsRows frame rows, walking the frame width
// in tiles of kFsTileW columns.
// A tile's rows (plus one halo row above and below, plus one halo column each side, reflect-101 at x = 0 / W-1) are staged as raw
// bytes in LDS with dword loads, converted to gray in LDS, and every lane then walks one column down the strip: full-frame counts
// for every row, the 3x3 Laplacian / Sobel for rows inside the band.  The band is an image of its own (cv2 receives a NumPy view),
// so the row above the band's first row is its second row (reflect-101), and the same at its last row; those rows always lie
// inside the staged window.  Sums go lane -> wavefront (cross-lane adds) -> workgroup (LDS) -> one 64-bit atomic per field.
//
// The same kernel with kEdge set is the edge pass (FS-EDGE v1): the default backend's score, the filter graph `format=gray,
// crop, signalstats, sobel, signalstats` of score_one_file_ffmpeg (FS:789-899).  Its strips cover the band only, the staging is the
// same code with libavfilter's mirror (one past the last row / column is the last one itself) in place of reflect-101, and every
// lane sums the gray and the clipped Sobel magnitude of its column into a gs360_frame_edge record.
//
// fs_small_kernel: the band resized with INTER_AREA (OpenCV's per-axis area tables, computed per output pixel in double exactly as
// computeResizeAreaTab does, float32 accumulation in ResizeArea_Invoker's order), and the gray at the INTER_NEAREST sample that the
// host turns into the resized valid mask.  A second, small launch over the band: its 2-D cells read every band pixel once more
// (the stats pass keeps to one streaming read of the frame), and it runs only for the fft / hybrid metrics.
#include <type_traits>

#include "gs360_framepx.h"

namespace gs360 {

namespace {

constexpr int kFsThreads = 256;
constexpr int kFsRows = 16;                    // frame rows per strip
constexpr int kFsTileW = 256;                  // columns per tile: one per lane
constexpr int kFsLdsRows = kFsRows + 2;        // + halo above and below
constexpr int kFsGrayPitch = 260;
constexpr int kFsFields = 13;                  // int64 fields of gs360_frame_stats
static_assert(sizeof(gs360_frame_stats) == kFsFields * 8, "gs360_frame_stats layout");

// T: the sample type, uint8_t or uint16_t (FS-DEPTH16 v1).  A staged row is (kFsTileW + 2) pixels of up to 4 samples + 3 bytes of
// alignment: 260 dwords of 8-bit samples, 520 of 16-bit ones, loaded in kLoads rounds of one dword per thread.
template <typename T>
struct FsLds {
    static constexpr int kRawDw = 260 * (int)sizeof(T);
    static constexpr int kLoads = (kRawDw + kFsThreads - 1) / kFsThreads;
    static_assert(((kFsTileW + 2) * 4 * (int)sizeof(T) + 3 + 3) / 4 <= kRawDw, "a staged row fits");
    uint32_t raw[kFsLdsRows][kRawDw];
    int32_t gray[kFsLdsRows][kFsGrayPitch];
    long long red[kFsThreads / 64][kFsFields];
};
static_assert(sizeof(FsLds<uint16_t>) <= 64 * 1024, "static LDS of one workgroup");

__device__ __forceinline__ int reflect101(int i, int n) {   // one step outside [0, n) at most (cv::borderInterpolate, BORDER_REFLECT_101)
    if (n == 1) return 0;
    return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
}

// libavfilter's 3x3 set-up, as FS-EDGE v1 restates it: |i| inside, else 2n - 1 - |i| (-1 -> 1, n -> n - 1; n = 1 -> 0)
__device__ __forceinline__ int mirror_av(int i, int n) {
    const int a = abs(i);
    return a < n ? a : 2 * n - 1 - a;
}

// floor(sqrt(s)) for 0 <= s < 2^24 (exact in float): the hardware square root is a candidate, integer compares settle it
__device__ __forceinline__ int isqrt24(int s) {
    int r = (int)__builtin_amdgcn_sqrtf((float)s);
    r -= r * r > s;
    r += (r + 1) * (r + 1) <= s;
    return r;
}

// The statistics pass takes the gray at full depth (g16 for uint16_t: sums in units of 1/257 gray level, 64-bit from the first
// product on); the edge pass takes the 8-bit view of the samples and is FS-EDGE v1 from there on.
template <int C, typename T, bool kEdge>
__global__ void __launch_bounds__(kFsThreads) fs_strip_kernel(const FsLaunch L) {
    using Lds = FsLds<T>;
    constexpr bool k16 = sizeof(T) == 2;
    constexpr int kPx = C * (int)sizeof(T);                 // bytes per pixel
    using Sum = std::conditional_t<k16, int64_t, int>;      // a lane's sums of g and lap: 4096 rows x 8 x 65535 passes 2^31
    using Sq = std::conditional_t<k16, int64_t, uint32_t>;  // a tile's sums of squares
    __shared__ Lds S;
    const int b = blockIdx.x;
    const int t = (b & 7) * L.chunk + (b >> 3);             // XCD-aware order: an XCD walks neighbouring strips (shared halo rows)
    if (t >= L.total) return;
    const int f = t / L.strips;
    const int H = L.H, W = L.W, y0 = L.y0, y1 = L.y1;
    const int ys = (kEdge ? y0 : 0) + (t - f * L.strips) * kFsRows;     // the edge pass walks the band's strips only
    const int ye = min(ys + kFsRows, kEdge ? y1 : H);
    const uint8_t* const src = L.src[f];
    const int tid = threadIdx.x;
    const int64_t r4 = circle_r4(W, H);

    int cnt_c = 0, cnt_h = 0, cnt_hc = 0;
    int n_a = 0, n_v = 0;
    Sum g_a = 0, l_a = 0, g_v = 0, l_v = 0;
    int64_t l2_a = 0, m2_a = 0, l2_v = 0, m2_v = 0;
    int e_a = 0;                                            // edge pass: sum of e, next to n_a and g_a (<= 256 tiles x kFsRows x 255)

    for (int x0 = 0; x0 < W; x0 += kFsTileW) {
        const int nx = min(kFsTileW, W - x0);
        const int xa = max(x0 - 1, 0), xb = min(x0 + nx, W - 1);    // staged pixel columns (the reflected halo lies inside)
        // 1. raw bytes of rows ys-1 .. ye (those the counts or a band stencil need) -> LDS, dword loads
        uint32_t v[kFsLdsRows][Lds::kLoads];
#pragma unroll
        for (int r = 0; r < kFsLdsRows; ++r) {
            const int y = ys - 1 + r;
            const bool need = y >= 0 && y < H && ((y >= ys && y < ye) || (y >= y0 && y < y1 && y <= ye));
            const uintptr_t a = (uintptr_t)(src + (int64_t)y * L.stride + xa * kPx);
            const uint32_t* q = (const uint32_t*)(a & ~(uintptr_t)3);
            const int ndw = need ? ((int)(a & 3) + (xb - xa + 1) * kPx + 3) >> 2 : 0;
#pragma unroll
            for (int k = 0; k < Lds::kLoads; ++k)
                v[r][k] = tid + k * kFsThreads < ndw ? __builtin_nontemporal_load(q + tid + k * kFsThreads) : 0u;
        }
#pragma unroll
        for (int r = 0; r < kFsLdsRows; ++r) {
#pragma unroll
            for (int k = 0; k < Lds::kLoads; ++k)
                if (tid + k * kFsThreads < Lds::kRawDw) S.raw[r][tid + k * kFsThreads] = v[r][k];
        }
        __syncthreads();
        // 2. gray of columns x0-1 .. x0+nx (reflect-101, or the edge pass's mirror, at the frame's left and right edges)
        for (int i = tid; i < kFsLdsRows * (kFsTileW + 2); i += kFsThreads) {
            const int r = i / (kFsTileW + 2), c = i - r * (kFsTileW + 2);
            if (c > nx + 1) continue;
            const int xs = kEdge ? mirror_av(x0 - 1 + c, W) : reflect101(x0 - 1 + c, W);
            const int off = (int)((uintptr_t)(src + (int64_t)(ys - 1 + r) * L.stride + xa * kPx) & 3);   // as staged in step 1
            const uint8_t* p = (const uint8_t*)S.raw[r] + off + (xs - xa) * kPx;
            S.gray[r][c] = kEdge ? gray8_of<C, T>(p, L.red) : gray_of<C, T>(p, L.red);
        }
        __syncthreads();
        // 3. one column per lane down the strip
        if constexpr (kEdge) {
            if (tid < nx) {
                // taps t[row][col] = wu / wm / wd; the band's row -1 is its row 1 (row 0 when it has one row), its row bh is row bh-1
                const int c = tid + 1;
                int wu[3], wm[3], wd[3];
                const int* Ru = S.gray[ys > y0 ? 0 : (y1 - y0 > 1 ? 2 : 1)] + c;
                const int* Rm = S.gray[1] + c;
#pragma unroll
                for (int k = 0; k < 3; ++k) { wu[k] = Ru[k - 1]; wm[k] = Rm[k - 1]; }
                for (int y = ys; y < ye; ++y) {
                    const int* Rd = S.gray[min(y + 1, y1 - 1) - ys + 1] + c;
#pragma unroll
                    for (int k = 0; k < 3; ++k) wd[k] = Rd[k - 1];
                    const int ga = (wd[0] + 2 * wd[1] + wd[2]) - (wu[0] + 2 * wu[1] + wu[2]);
                    const int gb = (wu[2] + 2 * wm[2] + wd[2]) - (wu[0] + 2 * wm[0] + wd[0]);
                    n_a += 1;
                    g_a += wm[1];
                    e_a += isqrt24(min(ga * ga + gb * gb, 255 * 255));            // min(255, floor(sqrt(.)))
#pragma unroll
                    for (int k = 0; k < 3; ++k) { wu[k] = wm[k]; wm[k] = wd[k]; }
                }
            }
        } else if (tid < nx) {
            const int c = tid + 1;
            const int x = x0 + tid;
            const int64_t dx = 2 * x - (W - 1);
            const int64_t dx2 = dx * dx;
            Sq tl2_a = 0, tm2_a = 0, tl2_v = 0, tm2_v = 0;         // 8-bit: <= kFsRows * 2040^2 < 2^32 per tile
            int wu[3], wm[3], wd[3];
            int pm = -2, pd = -2;                                   // band rows held in wm / wd
            for (int y = ys; y < ye; ++y) {
                const int64_t dy = 2 * y - (H - 1);
                const bool circ = dx2 + dy * dy <= r4;
                int g;
                const bool inband = y >= y0 && y < y1;
                if (inband) {
                    const int up = y > y0 ? y - 1 : (y1 - y0 > 1 ? y0 + 1 : y0);
                    const int dn = y < y1 - 1 ? y + 1 : (y1 - y0 > 1 ? y1 - 2 : y);
                    const int* Rd = S.gray[dn - ys + 1] + c;
                    if (up == pm && y == pd) {
#pragma unroll
                        for (int k = 0; k < 3; ++k) { wu[k] = wm[k]; wm[k] = wd[k]; }
                    } else {
                        const int* Ru = S.gray[up - ys + 1] + c;
                        const int* Rm = S.gray[y - ys + 1] + c;
#pragma unroll
                        for (int k = 0; k < 3; ++k) { wu[k] = Ru[k - 1]; wm[k] = Rm[k - 1]; }
                    }
#pragma unroll
                    for (int k = 0; k < 3; ++k) wd[k] = Rd[k - 1];
                    pm = y; pd = dn;
                    g = wm[1];
                } else {
                    g = S.gray[y - ys + 1][c];
                }
                const bool hl = g >= (k16 ? kFs16Highlight : 243);
                cnt_c += circ;
                cnt_h += hl;
                cnt_hc += hl && circ;
                if (inband) {
                    const int lap = 2 * (wu[0] + wu[2] + wd[0] + wd[2]) - 8 * wm[1];
                    const int gx = (wu[2] + 2 * wm[2] + wd[2]) - (wu[0] + 2 * wm[0] + wd[0]);
                    const int gy = (wd[0] + 2 * wd[1] + wd[2]) - (wu[0] + 2 * wu[1] + wu[2]);
                    // 16-bit: |lap| <= 8 * 65535 and |gx|, |gy| <= 4 * 65535, so the products need 64 bits
                    const Sq l2 = (Sq)((Sum)lap * lap), m2 = (Sq)((Sum)gx * gx + (Sum)gy * gy);
                    n_a += 1; g_a += g; l_a += lap; tl2_a += l2; tm2_a += m2;
                    const bool valid = (!L.circle || circ) && (!L.highlights || !hl);
                    if (valid) { n_v += 1; g_v += g; l_v += lap; tl2_v += l2; tm2_v += m2; }
                }
            }
            l2_a += tl2_a; m2_a += tm2_a; l2_v += tl2_v; m2_v += tm2_v;
        }
        __syncthreads();
    }
    // lane -> wavefront -> workgroup -> one atomic per field of the frame's record
    constexpr int kN = kEdge ? 3 : kFsFields;
    static_assert(sizeof(gs360_frame_edge) == 3 * 8, "gs360_frame_edge layout");
    long long acc[kN];
    if constexpr (kEdge) {
        acc[0] = wave_sum(n_a); acc[1] = wave_sum(g_a); acc[2] = wave_sum(e_a);
    } else {
        const long long all[kFsFields] = {wave_sum(cnt_c), wave_sum(cnt_h), wave_sum(cnt_hc),
                                          wave_sum(n_a), wave_sum(g_a), wave_sum(l_a), wave_sum((long long)l2_a), wave_sum((long long)m2_a),
                                          wave_sum(n_v), wave_sum(g_v), wave_sum(l_v), wave_sum((long long)l2_v), wave_sum((long long)m2_v)};
#pragma unroll
        for (int k = 0; k < kFsFields; ++k) acc[k] = all[k];
    }
    unsigned long long* const rec = kEdge ? (unsigned long long*)&L.edge[f] : (unsigned long long*)&L.stats[f];
    const int wave = tid >> 6;
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < kN; ++k) S.red[wave][k] = acc[k];
    }
    __syncthreads();
    if (tid < kN) {
        long long s = 0;
#pragma unroll
        for (int w = 0; w < kFsThreads / 64; ++w) s += S.red[w][tid];
        if (s != 0) atomicAdd(rec + tid, (unsigned long long)s);
    }
}

template <int C, typename T>
__global__ void __launch_bounds__(kFsThreads) fs_small_kernel(const FsLaunch L) {
    const int dx = blockIdx.x * kFsThreads + threadIdx.x;
    const int dy = blockIdx.y;
    const int f = blockIdx.z;
    if (dx >= L.small_w) return;
    const int bh = L.y1 - L.y0;
    const uint8_t* const band = L.src[f] + (int64_t)L.y0 * L.stride;
    const AreaSpan ax = area_span(dx, L.W, L.scale_x);
    const AreaSpan ay = area_span(dy, bh, L.scale_y);
    float sum = 0.0f;                                        // sum[dx] += beta * buf[dx], ytab order
    if (ay.has_head) sum += ay.head * area_row<C, T>(band + (int64_t)(ay.i1 - 1) * L.stride, ax, L.red);
    for (int sy = ay.i1; sy < ay.i2; ++sy) sum += ay.mid * area_row<C, T>(band + (int64_t)sy * L.stride, ax, L.red);
    if (ay.has_tail) sum += ay.tail * area_row<C, T>(band + (int64_t)ay.i2 * L.stride, ax, L.red);
    const int nx = nearest_index(dx, L.scale_x, L.W);
    const int ny = nearest_index(dy, L.scale_y, bh);
    float* out = L.small[f];
    const int64_t plane = (int64_t)L.small_w * L.small_h;
    out[(int64_t)dy * L.small_w + dx] = sum;
    out[plane + (int64_t)dy * L.small_w + dx] = gray_level<C, T>(band + (int64_t)ny * L.stride + nx * C * (int)sizeof(T), L.red);
}

template <int C, typename T>
hipError_t launch_fs(FsLaunch& L, hipStream_t s) {
    L.strips = (L.H + kFsRows - 1) / kFsRows;
    L.total = L.strips * L.n_frames;
    L.chunk = (L.total + 7) / 8;
    hipLaunchKernelGGL((fs_strip_kernel<C, T, false>), dim3((unsigned)(L.chunk * 8)), dim3(kFsThreads), 0, s, L);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !L.small[0]) return e;
    hipLaunchKernelGGL((fs_small_kernel<C, T>), dim3((unsigned)((L.small_w + kFsThreads - 1) / kFsThreads), (unsigned)L.small_h,
                                                     (unsigned)L.n_frames), dim3(kFsThreads), 0, s, L);
    return hipGetLastError();
}

template <int C, typename T>
hipError_t launch_fe(FsLaunch& L, hipStream_t s) {
    L.strips = (L.y1 - L.y0 + kFsRows - 1) / kFsRows;
    L.total = L.strips * L.n_frames;
    L.chunk = (L.total + 7) / 8;
    hipLaunchKernelGGL((fs_strip_kernel<C, T, true>), dim3((unsigned)(L.chunk * 8)), dim3(kFsThreads), 0, s, L);
    return hipGetLastError();
}

// One of the per-channel-count, per-sample-type instantiations of a launcher
template <typename T>
hipError_t launch_fs_c(FsLaunch& L, hipStream_t s) {
    switch (L.C) {
        case 1: return launch_fs<1, T>(L, s);
        case 3: return launch_fs<3, T>(L, s);
        case 4: return launch_fs<4, T>(L, s);
        default: return hipErrorInvalidValue;
    }
}
template <typename T>
hipError_t launch_fe_c(FsLaunch& L, hipStream_t s) {
    switch (L.C) {
        case 1: return launch_fe<1, T>(L, s);
        case 3: return launch_fe<3, T>(L, s);
        case 4: return launch_fe<4, T>(L, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_frame_stats(FsLaunch& L, hipStream_t s) {
    return L.depth == 16 ? launch_fs_c<uint16_t>(L, s) : launch_fs_c<uint8_t>(L, s);
}

hipError_t launch_frame_edge(FsLaunch& L, hipStream_t s) {
    return L.depth == 16 ? launch_fe_c<uint16_t>(L, s) : launch_fe_c<uint8_t>(L, s);
}

}  // namespace gs360
