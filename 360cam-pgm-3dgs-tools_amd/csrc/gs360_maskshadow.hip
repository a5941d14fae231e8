// gs360_maskshadow.hip -- the shadow estimate in front of the mask-finishing chain (MSK-SHADOW v1).
//
// Reference: gs360_SegmentationMaskTool.py's estimate_shadow_mask (SEG:499-558): pixels much darker than a wide Gaussian of the gray
// image, of low saturation, near the person mask, cleaned by a close and an open, kept per outer contour of enough area and filled.
// The morphology is gs360_maskmorph.hip's mk_morph_kernel (launched by the glue); the steps on a plane that both files share (a bit,
// the 4-byte group store, the gathered word, the ballot as two dwords, the count tail, the atomics) and every step's launch geometry
// are gs360_maskplane.h's; this file holds the rest:
//
//   pixel     four pixels per lane: gray (gray_of) as one dword of the gray plane, `S <= sat_max` (cv2's 8-bit RGB2HSV, the divisor
//             table is DATA) as a nibble; eight lanes' nibbles are shuffled into a dword of the plane, as mk_pack_kernel packs
//   rows      a workgroup stages 2048 gray pixels of a row and r more on either side, reflected (BORDER_REFLECT_101) while staging,
//             as floats in LDS; a lane produces eight neighbouring outputs and keeps their left and right taps in two register
//             windows that slide one place per tap: two LDS reads per tap for eight outputs.  The LDS index is skewed by one
//             place per 32 so that lanes eight floats apart read different banks.  The weights k[0 .. r] are DATA.
//   cols      lanes along x; a workgroup stages 128 + 2 r rows of 64 columns of the row pass's plane, reflected in y; a wave owns
//             32 of the rows, eight at a time with the same sliding windows.  Fused with the candidate test: the wave's 64 bits of
//             C0 per row are one ballot, stored as two dwords.  The blurred plane is never stored.
//   logic     out = a & b & ~c on planes
//   label     union-find by label equivalence over a bit plane (or its complement), connectivity 4 or 8: `init` gives a pixel the
//             index of the start of its run inside its dword, `merge` links (atomicMin on roots) the runs of neighbouring dwords
//             and, per run of overlap, a row to the row above, `flatten` points every pixel at its root (one walk per run).  No
//             lane waits for another one; every walk and retry is bounded by H W and sets the launch's error word past that.
//   border    flags the roots of the background components that touch the image border; fill: G = not (background under such a root)
//   area      a lane owns the 32 cells of a dword column over 16 cell rows: per run of contributing cells one lookup of the root,
//             and one integer atomic add on area[root] whenever the root changes (a filled blob costs one per lane)
//   select    clean = G and area[root] >= 2 th; M = P | clean as bytes of 0 / 255 (four pixels per lane), the clean plane, the count
//
// Floating point is taken op by op (the library is built with -ffp-contract=off; no fma here).  The per-lane arithmetic is
// host-callable (MK_HD) so that tests/tools/maskshadow_hostcheck.hip can step it under a sanitizer.
#include "gs360_maskplane.h"

#pragma clang fp contract(off)

namespace gs360 {
namespace {

MK_HD inline int64_t ms_gray_pitch(const MsJob& J) { return 32 * (int64_t)J.pw; }

// ---- pixel -----------------------------------------------------------------------------------------------------------------------
// four pixels from column x (a multiple of 4) on: their grays as the bytes of a dword, `S <= sat_max` as a nibble; zero at columns >= W
MK_HD inline void ms_pixel4(const MsJob& J, int y, int x, uint32_t* gray4, uint32_t* nib) {
    *gray4 = 0; *nib = 0;
    if (x >= J.W) return;
    const uint8_t* p = J.img + (int64_t)y * J.img_stride + 3 * (int64_t)x;
    uint32_t w[3] = {0, 0, 0};
    if (x + 4 <= J.W && ((uintptr_t)p & 3) == 0) __builtin_memcpy(w, __builtin_assume_aligned(p, 4), 12);
    else
        for (int b = 0; b < 12 && x + b / 3 < J.W; ++b) w[b >> 2] |= (uint32_t)p[b] << (8 * (b & 3));
    for (int k = 0; k < 4 && x + k < J.W; ++k) {
        uint8_t px[3];
        for (int c = 0; c < 3; ++c) px[c] = (uint8_t)(w[(3 * k + c) >> 2] >> (8 * ((3 * k + c) & 3)));
        const int v = mk_hi(mk_hi(px[0], px[1]), px[2]), d = v - mk_lo(mk_lo(px[0], px[1]), px[2]);
        const int S = (d * J.sdiv[v] + 2048) >> 12;
        *gray4 |= (uint32_t)gray_of<3>(px, 0) << (8 * k);
        *nib |= (uint32_t)(S <= J.sat_max) << k;
    }
}

// ---- blur ------------------------------------------------------------------------------------------------------------------------
// BORDER_REFLECT_101 for any p: reflections at 0 and len - 1 repeat with period 2 (len - 1)
MK_HD inline int ms_reflect(int p, int len) {
    if (len == 1) return 0;
    const int period = 2 * (len - 1);
    int m = p % period;
    if (m < 0) m += period;
    return m < len ? m : period - m;
}
// eight neighbouring outputs from position c0 on: s = k[0] v(c); s = s + k[i] (v(c - i) + v(c + i)) for i = 1 .. r, every operation
// rounded on its own.  lw[j] = v(c0 + j - i), rw[j] = v(c0 + j + i): each step shifts the windows and reads one new value each.
template <class At>
MK_HD inline void ms_filter(const At& at, int c0, const float* k, int r, float* out) {
    float lw[kMsOut], rw[kMsOut];
    const float k0 = k[0];
#pragma unroll
    for (int j = 0; j < kMsOut; ++j) { lw[j] = rw[j] = at(c0 + j); out[j] = k0 * lw[j]; }
    for (int i = 1; i <= r; ++i) {
#pragma unroll
        for (int j = kMsOut - 1; j > 0; --j) lw[j] = lw[j - 1];
        lw[0] = at(c0 - i);
#pragma unroll
        for (int j = 0; j < kMsOut - 1; ++j) rw[j] = rw[j + 1];
        rw[kMsOut - 1] = at(c0 + kMsOut - 1 + i);
        const float ki = k[i];
#pragma unroll
        for (int j = 0; j < kMsOut; ++j) out[j] = out[j] + ki * (lw[j] + rw[j]);
    }
}
MK_HD inline int ms_round_up8(int v) { return (v + 7) & ~7; }

// the row pass: a workgroup's segment of row y from column x0 (a multiple of kMsRowSeg) on
MK_HD inline int ms_skew(int e) { return e + (e >> 5); }
MK_HD inline int ms_rows_len(const MsJob& J, int x0) { return mk_lo(kMsRowSeg, ms_round_up8(J.W - x0)); }      // outputs computed
constexpr int kMsRowStage = kMsRowSeg + 2 * kMsMaxR + (kMsRowSeg + 2 * kMsMaxR) / 32 + 1;
MK_HD inline void ms_rows_stage(const MsJob& J, int y, int x0, int lane, float* stage) {
    const int n = ms_rows_len(J, x0) + 2 * J.r;
    const uint8_t* row = J.gray + (int64_t)y * ms_gray_pitch(J);
    for (int e = lane; e < n; e += kMsThreads) stage[ms_skew(e)] = (float)row[ms_reflect(x0 - J.r + e, J.W)];
}
MK_HD inline void ms_rows_lane(const MsJob& J, int y, int x0, int lane, const float* stage) {
    const int c0 = kMsOut * lane, r = J.r;
    if (x0 + c0 >= J.W) return;
    float out[kMsOut];
    ms_filter([&](int c) { return stage[ms_skew(c + r)]; }, c0, J.k, r, out);
    float* dst = J.mid + (int64_t)y * J.W + x0 + c0;
    for (int j = 0; j < kMsOut && x0 + c0 + j < J.W; ++j) dst[j] = out[j];
}

// the column pass: a workgroup's tile of kMsColW columns from x0 and kMsColRows rows from y0
MK_HD inline int ms_cols_rows(const MsJob& J, int y0) { return mk_lo(kMsColRows, ms_round_up8(J.H - y0)) + 2 * J.r; }   // staged rows
MK_HD inline void ms_cols_stage(const MsJob& J, int y0, int x0, int lane, float* stage) {
    const int n = ms_cols_rows(J, y0) * kMsColW;
    for (int idx = lane; idx < n; idx += kMsThreads) {
        const int rr = idx / kMsColW, x = x0 + (idx - rr * kMsColW);
        stage[idx] = x < J.W ? J.mid[(int64_t)ms_reflect(y0 - J.r + rr, J.H) * J.W + x] : 0.0f;
    }
}
// step 3 at pixel (y, x) with its blurred gray
MK_HD inline bool ms_candidate(const MsJob& J, int y, int x, float illum) {
    const float g = (float)J.gray[(int64_t)y * ms_gray_pitch(J) + x];
    const float ratio = g / (illum + 1e-6f), delta = illum - g;
    return ratio < J.t && delta >= J.delta_min && mk_bit(J.a, J.pw, y, x);
}
// lane's column, rows c0 .. c0 + 7 of the tile (c0 = 32 wave + 8 chunk, below H - y0) -> bit j: the candidate test of row y0 + c0 + j
MK_HD inline uint32_t ms_cols_lane(const MsJob& J, int y0, int x0, int lane, int c0, const float* stage) {
    const int xl = lane & (kMsColW - 1), x = x0 + xl, r = J.r;
    float out[kMsOut];
    ms_filter([&](int c) { return stage[(c + r) * kMsColW + xl]; }, c0, J.k, r, out);
    uint32_t bits = 0;
    for (int j = 0; j < kMsOut; ++j)
        if (x < J.W && y0 + c0 + j < J.H) bits |= (uint32_t)ms_candidate(J, y0 + c0 + j, x, out[j]) << j;
    return bits;
}

// ---- labels ----------------------------------------------------------------------------------------------------------------------
MK_HD inline void ms_fail(uint32_t* err) { *err = 1u; }
// dword w of row y of the plane that is labelled; zero outside it
MK_HD inline uint32_t ms_label_bits(const MsJob& J, int y, int w) {
    if (y < 0 || w < 0 || w >= J.pw) return 0;
    const uint32_t v = J.a[(int64_t)y * J.pw + w];
    return (J.flags & kMsComplement) ? ~v & mk_colmask(J.W, w) : v;
}
// the root of x.  A parent is never above its child, so a chain is shorter than the plane: H W steps bound the walk; a value
// that is no index of the plane ends it as well.
MK_HD inline int32_t ms_root(const MsJob& J, int32_t x, uint32_t* err) {
    const int32_t bound = J.H * J.W;
    for (int32_t n = 0; n < bound; ++n) {
        const int32_t p = mk_atomic_load(J.lab + x);
        if (p == x) return x;
        if ((uint32_t)p >= (uint32_t)bound) break;
        x = p;
    }
    ms_fail(err);
    return x;
}
// one set for a and b: the larger root is pointed at the smaller one.  Where another lane has linked that root first, the link it
// made (old) and b are joined next; old is below a, so H W retries bound the loop.
MK_HD inline void ms_unite(const MsJob& J, int32_t a, int32_t b, uint32_t* err) {
    const int32_t bound = J.H * J.W;
    for (int32_t n = 0; n < bound; ++n) {
        a = ms_root(J, a, err); b = ms_root(J, b, err);
        if (a == b) return;
        if (a < b) { const int32_t t = a; a = b; b = t; }
        const int32_t old = mk_atomic_min(J.lab + a, b);
        if (old == a) return;
        a = old;
    }
    ms_fail(err);
}
// item q = dword (y, w): a set pixel's label is the index of the first pixel of its run inside the dword, any other pixel's -1
MK_HD inline void ms_label_init(const MsJob& J, int64_t q) {
    const int y = (int)(q / J.pw), w = (int)(q - (int64_t)y * J.pw), nx = mk_lo(32, J.W - 32 * w);
    const uint32_t m = ms_label_bits(J, y, w);
    const int32_t base = y * J.W + 32 * w;
    int start = 0;
    for (int b = 0; b < nx; ++b) {
        const bool set = (m >> b) & 1u;
        if (set && (b == 0 || !((m >> (b - 1)) & 1u))) start = b;
        J.lab[base + b] = set ? base + start : -1;
    }
}
// item q = dword (y, w): its first pixel to the run that ends the dword on the left; per run of pixels set here and straight above, the
// first of them to the pixel above; with connectivity 8 a pixel whose upper neighbour is clear to the upper diagonal ones, unless the
// pixel beside it links the same two runs
template <int CONN>
MK_HD inline void ms_label_merge(const MsJob& J, int64_t q, uint32_t* err) {
    const int y = (int)(q / J.pw), w = (int)(q - (int64_t)y * J.pw), W = J.W;
    const uint32_t cur = ms_label_bits(J, y, w);
    if (!cur) return;
    const uint32_t cl = ms_label_bits(J, y, w - 1) >> 31, cr = ms_label_bits(J, y, w + 1) & 1u;
    const uint32_t up = ms_label_bits(J, y - 1, w), ul = ms_label_bits(J, y - 1, w - 1) >> 31, ur = ms_label_bits(J, y - 1, w + 1) & 1u;
    const int32_t base = y * W + 32 * w;
    if ((cur & 1u) && cl) ms_unite(J, base, base - 1, err);
    const uint32_t v = cur & up;
    for (uint32_t m = v & ~((v << 1) | (cl & ul)); m; m &= m - 1) ms_unite(J, base + mk_ctz(m), base + mk_ctz(m) - W, err);
    if (CONN == 8) {
        const uint32_t curm1 = (cur << 1) | cl, curp1 = (cur >> 1) | (cr << 31), upm1 = (up << 1) | ul, upp1 = (up >> 1) | (ur << 31);
        for (uint32_t m = cur & upm1 & ~up & ~curm1; m; m &= m - 1) ms_unite(J, base + mk_ctz(m), base + mk_ctz(m) - W - 1, err);
        for (uint32_t m = cur & upp1 & ~up & ~curp1; m; m &= m - 1) ms_unite(J, base + mk_ctz(m), base + mk_ctz(m) - W + 1, err);
    }
}
// item q = dword (y, w): the pixels of a run inside the dword still name the run's first pixel (only roots are ever relinked), so one
// walk from there serves the run
MK_HD inline void ms_label_flatten(const MsJob& J, int64_t q, uint32_t* err) {
    const int y = (int)(q / J.pw), w = (int)(q - (int64_t)y * J.pw);
    const int32_t base = y * J.W + 32 * w;
    for (uint32_t m = ms_label_bits(J, y, w); m;) {
        const int s = mk_ctz(m);
        const uint32_t run = m & ~(m + (1u << s));       // the carry runs through the run that starts at bit s
        const int32_t root = ms_root(J, base + s, err);
        for (uint32_t b = run; b; b &= b - 1) J.lab[base + mk_ctz(b)] = root;
        m &= ~run;
    }
}
// item q = a pixel of the four border lines (ms_border_items): the root of a labelled one is flagged (equal stores, in any order)
MK_HD inline void ms_border(const MsJob& J, int64_t q) {
    const int W = J.W, H = J.H;
    const int64_t p = q < W ? q : q < 2 * W ? (int64_t)(H - 1) * W + (q - W) : q < 2 * W + H ? (q - 2 * W) * W : (q - 2 * W - H) * W + W - 1;
    const int32_t l = J.lab[p];
    if (l >= 0) J.area[l] = 1u;
}
// G at (y, x): everything but the labelled (background) pixels under a flagged root
MK_HD inline bool ms_fill_bit(const MsJob& J, int y, int x) {
    const int32_t l = J.lab[(int64_t)y * J.W + x];
    return !(l >= 0 && J.area[l]);
}

// ---- area ------------------------------------------------------------------------------------------------------------------------
// item q (ms_area_items) = (band of kMsAreaRows cell rows, dword column w).  Cell (y, x) has the corners (y, x), (y, x + 1), (y + 1, x), (y + 1, x + 1);
// it adds 2 with four corners in G and 1 with three.  Neighbouring contributing cells share a set corner or two vertically adjacent
// ones, so a run of them has one root: one lookup per run, one atomic whenever the root changes.
MK_HD inline void ms_area_lane(const MsJob& J, int64_t q, uint32_t* err) {
    const int band = (int)(q / J.pw), w = (int)(q - (int64_t)band * J.pw), pw = J.pw;
    const int y1 = mk_lo((band + 1) * kMsAreaRows, J.H - 1);
    int32_t root = -1;
    uint32_t sum = 0;
    for (int y = band * kMsAreaRows; y < y1; ++y) {
        const uint32_t* g = J.a + (int64_t)y * pw + w;
        const uint32_t a = g[0], b = g[pw], an = w + 1 < pw ? g[1] & 1u : 0u, bn = w + 1 < pw ? g[pw + 1] & 1u : 0u;
        const uint32_t a1 = (a >> 1) | (an << 31), b1 = (b >> 1) | (bn << 31);
        const uint32_t four = a & a1 & b & b1;
        const uint32_t three = (a & a1 & b & ~b1) | (a & a1 & ~b & b1) | (a & ~a1 & b & b1) | (~a & a1 & b & b1);
        uint32_t todo = four | three;
        while (todo) {
            const int s = mk_ctz(todo);
            const uint32_t gap = ~(todo >> s);
            const int n = gap ? mk_ctz(gap) : 32;
            const uint32_t run = (n >= 32 ? 0xffffffffu : (1u << n) - 1u) << s;
            const int32_t at = (((a >> s) & 1u) ? y : y + 1) * J.W + 32 * w + s;      // a set corner of the run's first cell
            const int32_t l = J.lab[at];
            if (l < 0) { ms_fail(err); return; }
            if (l != root) {
                if (sum) mk_atomic_add(J.area + root, sum);
                root = l; sum = 0;
            }
            sum += 2u * (uint32_t)mk_popc(four & run) + (uint32_t)mk_popc(three & run);
            todo &= ~run;
        }
    }
    if (sum) mk_atomic_add(J.area + root, sum);
}

// ---- select ----------------------------------------------------------------------------------------------------------------------
// four pixels from column x (a multiple of 4) on: the clean nibble; M = P | clean goes out as bytes and comes back as a nibble
MK_HD inline void ms_select4(const MsJob& J, int y, int x, uint32_t* clean, uint32_t* merged) {
    *clean = 0; *merged = 0;
    if (x >= J.W) return;
    uint32_t v = 0;
    for (int k = 0; k < 4 && x + k < J.W; ++k) {
        const bool c = mk_bit(J.a, J.pw, y, x + k) && J.area[J.lab[(int64_t)y * J.W + x + k]] >= J.th2;
        const bool m = c || mk_bit(J.b, J.pw, y, x + k);
        *clean |= (uint32_t)c << k; *merged |= (uint32_t)m << k;
        v |= (m ? 255u : 0u) << (8 * k);
    }
    mk_store4(J.dst + (int64_t)y * J.dst_stride + x, x, J.W, v);
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ const MsJob& ms_job(const MsLaunch& L, int* j) {
    *j = job_of(L, blockIdx.x, &MsJob::tile_base);
    return L.job[*j];
}

__global__ void __launch_bounds__(kMsThreads) ms_pixel_kernel(const MsLaunch L) {
    int j, y, tx;
    const MsJob& J = ms_job(L, &j);
    mk_tile_of(J, &y, &tx);
    const int x = tx * kMsPixelTile.w + 4 * threadIdx.x;
    uint32_t gray4, nib;
    ms_pixel4(J, y, x, &gray4, &nib);
    const uint32_t word = mk_gather8(nib);
    if (x >= 32 * J.pw) return;
    *(uint32_t*)(J.gray + (int64_t)y * ms_gray_pitch(J) + x) = gray4;
    mk_store_word(J.out, J.pw, y, x, word);
}

__global__ void __launch_bounds__(kMsThreads) ms_blur_rows_kernel(const MsLaunch L) {
    __shared__ float stage[kMsRowStage];
    int j, y, tx;
    const MsJob& J = ms_job(L, &j);
    mk_tile_of(J, &y, &tx);
    ms_rows_stage(J, y, tx * kMsRowsTile.w, threadIdx.x, stage);
    __syncthreads();
    ms_rows_lane(J, y, tx * kMsRowsTile.w, threadIdx.x, stage);
}

__global__ void __launch_bounds__(kMsThreads) ms_blur_cols_kernel(const MsLaunch L) {
    extern __shared__ float ms_cols_stage_lds[];         // (kMsColRows + 2 r) rows of kMsColW floats, r the launch's largest
    int j, ty, tx;
    const MsJob& J = ms_job(L, &j);
    mk_tile_of(J, &ty, &tx);
    const int y0 = ty * kMsColsTile.h, x0 = tx * kMsColsTile.w;
    ms_cols_stage(J, y0, x0, threadIdx.x, ms_cols_stage_lds);
    __syncthreads();
    const int wave = threadIdx.x / kMsColW, x = x0 + (threadIdx.x & (kMsColW - 1));
    for (int chunk = 0; chunk < kMsColRows / 4 / kMsOut; ++chunk) {
        const int c0 = wave * (kMsColRows / 4) + chunk * kMsOut;
        if (y0 + c0 >= J.H) break;                        // (the same for the whole wave)
        const uint32_t bits = ms_cols_lane(J, y0, x0, threadIdx.x, c0, ms_cols_stage_lds);
        for (int k = 0; k < kMsOut && y0 + c0 + k < J.H; ++k) mk_store_ballot(J.out, J.pw, y0 + c0 + k, x, (bits >> k) & 1u);
    }
}

__global__ void __launch_bounds__(kMsThreads) ms_logic_kernel(const MsLaunch L) {
    int j;
    const MsJob& J = ms_job(L, &j);
    const int64_t q = mk_item_of(J);
    if (q < mk_plane_items(J)) J.out[q] = J.a[q] & J.b[q] & ~J.c[q];
}

template <int STEP>
__global__ void __launch_bounds__(kMsThreads) ms_label_kernel(const MsLaunch L) {
    int j;
    const MsJob& J = ms_job(L, &j);
    const int64_t q = mk_item_of(J);
    if (STEP == 0) { if (q < mk_plane_items(J)) ms_label_init(J, q); }
    else if (STEP == 4) { if (q < mk_plane_items(J)) ms_label_merge<4>(J, q, L.err); }
    else if (STEP == 8) { if (q < mk_plane_items(J)) ms_label_merge<8>(J, q, L.err); }
    else if (STEP == 1) { if (q < mk_plane_items(J)) ms_label_flatten(J, q, L.err); }
    else if (STEP == 2) { if (q < ms_border_items(J)) ms_border(J, q); }
    else if (q < ms_area_items(J)) ms_area_lane(J, q, L.err);
}

__global__ void __launch_bounds__(kMsThreads) ms_fill_kernel(const MsLaunch L) {
    int j, y, tx;
    const MsJob& J = ms_job(L, &j);
    mk_tile_of(J, &y, &tx);
    const int x = tx * kMsFillTile.w + threadIdx.x;
    mk_store_ballot(J.out, J.pw, y, x, x < J.W && ms_fill_bit(J, y, x));
}

__global__ void __launch_bounds__(kMsThreads) ms_select_kernel(const MsLaunch L) {
    int j, band, tx;
    const MsJob& J = ms_job(L, &j);
    mk_tile_of(J, &band, &tx);
    const int x = tx * kMsSelectTile.w + 4 * threadIdx.x, y1 = min(J.H, (band + 1) * kMsSelectTile.h);
    uint32_t n = 0;
    for (int y = band * kMsSelectTile.h; y < y1; ++y) {
        uint32_t clean, merged;
        ms_select4(J, y, x, &clean, &merged);
        mk_store_word(J.out, J.pw, y, x, mk_gather8(clean));
        n += (uint32_t)__popc(merged);
    }
    mk_count_tail(n, L.counts + j);
}

}  // namespace

hipError_t launch_mask_shadow(MsStep step, const MsLaunch& L, hipStream_t s) {
    switch (step) {
    case kMsPixel: return mk_launch(ms_pixel_kernel, L, s);
    case kMsBlurRows: return mk_launch(ms_blur_rows_kernel, L, s);
    case kMsBlurCols: {
        int r = 0;
        for (int k = 0; k < L.n_jobs; ++k) r = L.job[k].r > r ? L.job[k].r : r;
        const size_t lds = (size_t)(kMsColRows + 2 * r) * kMsColW * sizeof(float);    // at most 163 328 bytes of the CU's 160 KiB
        hipError_t e = hipFuncSetAttribute((const void*)ms_blur_cols_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        return e != hipSuccess ? e : mk_launch(ms_blur_cols_kernel, L, s, lds);
    }
    case kMsLogic: return mk_launch(ms_logic_kernel, L, s);
    case kMsLabelInit: return mk_launch(ms_label_kernel<0>, L, s);
    case kMsLabelMerge: return L.conn == 8 ? mk_launch(ms_label_kernel<8>, L, s) : mk_launch(ms_label_kernel<4>, L, s);
    case kMsLabelFlatten: return mk_launch(ms_label_kernel<1>, L, s);
    case kMsBorder: return mk_launch(ms_label_kernel<2>, L, s);
    case kMsFill: return mk_launch(ms_fill_kernel, L, s);
    case kMsArea: return mk_launch(ms_label_kernel<3>, L, s);
    case kMsSelect: return mk_launch(ms_select_kernel, L, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace gs360
