// gs360_maskmorph.hip -- the finishing chain of segmentation masks on the device (MSK-SPEC v1).
//
// Reference: gs360_SegmentationMaskTool.py's process_loaded_sample after the network (SEG:680-781): close with an ellipse, dilate
// with a larger one, fuse to the frame edges, OR in the manual add layer, count, compose.  A mask is a bit plane here (bit x & 31 of
// dword x >> 5), so a dilation is shifts and ORs on 32 pixels at once; the arithmetic is integer and exact (tests/maskfinish_np.py).
//
//   pack     one lane per four pixels (a dword load): `value > thresh`; eight lanes' nibbles are shuffled into a dword of the plane
//   morph    one dilate or erode by an element given as DATA (per element row a half-open span of columns, device memory).  A
//            workgroup owns 32 dwords x 32 rows of output; it stages the rows and halo dwords a band of element rows reaches in LDS
//            and every lane keeps four output dwords in registers: per element row the OR over the span's window of one staged row
//            (windows up to 32 wide: log-step shift-ORs on 64 bits; wider ones: a suffix smear of the first 31 bits, a prefix smear
//            of the last 31 and "any bit" of the span all 32 windows share).  Elements taller than a band take several bands into
//            the same registers: no atomics, no order between workgroups.  An erode is the same launch with the plane complemented on
//            the way in and out (inside the image only): outside pixels never restrict it.
//   fuse     phase 0 copies the plane; phase 1 ORs the four strips' fills into the copy (one lane per dword column of the top and
//            bottom strip, one per row of the left and right strip; integer atomic ORs, which commute)
//   finish   phase 0 ORs the add layer into the plane and counts: four pixels per lane over a band of 32 rows, a wave reduction, one
//            atomic per workgroup (a mask has one counter: few workgroups per mask keep it from serialising the pass); phase 1
//            writes the mask (four pixels per lane) or composes RGBA / keep / remove (one), and takes the
//            empty-mask branches from the count
// Every loop is bounded by H, W, kh or the strip; there are no waits between workgroups.  The per-lane arithmetic is host-callable
// (MK_HD) so that tests/tools/maskmorph_hostcheck.hip can step it under a sanitizer.  The steps on a plane that the shadow estimate
// shares (a bit, a nibble, the 4-byte group load and store, the gathered word, the count tail, the atomics) and every step's launch
// geometry are gs360_maskplane.h's; this file holds the morph, fuse and compose arithmetic.
#include "gs360_maskplane.h"

namespace gs360 {
namespace {

// ---- pack ------------------------------------------------------------------------------------------------------------------------
// four pixels of a byte plane from column x (a multiple of 4) on as a nibble: bit k = `value > thresh`; clear at columns >= W and for a
// plane that is not there
MK_HD inline uint32_t mk_nibble(const uint8_t* plane, int64_t stride, int W, int thresh, int y, int x) {
    if (!plane || x >= W) return 0;
    const uint32_t v = mk_load4(plane + (int64_t)y * stride + x, x, W);
    uint32_t nib = 0;
    for (int k = 0; k < 4; ++k) nib |= (uint32_t)((int)((v >> (8 * k)) & 255u) > thresh) << k;
    return nib;
}

// ---- morph -----------------------------------------------------------------------------------------------------------------------
// element row i -> the staged row offset dy and the window [lo, hi] of columns relative to the output pixel; false: an empty span
MK_HD inline bool mk_span(const MkJob& J, int i, int* dy, int* lo, int* hi) {
    const int j1 = J.spans[2 * i], j2 = J.spans[2 * i + 1];
    *dy = i - J.ay; *lo = j1 - J.ax; *hi = j2 - 1 - J.ax;
    return j2 > j1;
}
// staged dword idx of a band: rows y0 + dlo .. of the plane, dwords w0 - halo .., zero outside the plane
MK_HD inline uint32_t mk_stage_word(const MkJob& J, int y0, int w0, int dlo, int sw, int idx) {
    const int r = idx / sw, c = idx - r * sw;
    const int y = y0 + dlo + r, w = w0 - J.halo + c;
    if (y < 0 || y >= J.H || w < 0 || w >= J.pw) return 0;
    const uint32_t v = J.in[(int64_t)y * J.pw + w];
    return (J.flags & kMkCompIn) ? ~v & mk_colmask(J.W, w) : v;
}
// 32 bits of a staged row from bit p on
MK_HD inline uint32_t mk_bits_at(const uint32_t* row, int p) {
    const int k = p >> 5, sh = p & 31;
    return (uint32_t)((((uint64_t)row[k + 1] << 32) | row[k]) >> sh);
}
// OR over d in [lo, hi] of the staged row shifted down by d, at dword wl: bit b = any of the row's bits 32 wl + b + lo .. + hi
MK_HD inline uint32_t mk_row_or(const uint32_t* row, int wl, int lo, int hi) {
    const int len = hi - lo + 1, p = 32 * wl + lo;
    if (len <= 32) {
        const int k = p >> 5, sh = p & 31;
        uint64_t v = (((uint64_t)row[k + 1] << 32) | row[k]) >> sh;
        if (sh) v |= (uint64_t)row[k + 2] << (64 - sh);
        int n = 1;
        for (; 2 * n <= len; n *= 2) v |= v >> n;        // windows of 1, 2, 4, ... compose exactly
        v |= v >> (len - n);
        return (uint32_t)v;
    }
    uint32_t head = mk_bits_at(row, p) & 0x7fffffffu;    // bits b + lo .. 30 + lo: a suffix OR
    head |= head >> 1; head |= head >> 2; head |= head >> 4; head |= head >> 8; head |= head >> 16;
    uint32_t tail = mk_bits_at(row, p + len) << 1;       // bits hi + 1 .. hi + b: a prefix OR
    tail |= tail << 1; tail |= tail << 2; tail |= tail << 4; tail |= tail << 8; tail |= tail << 16;
    const int a = p + 31, b = p + len - 1, ka = a >> 5, kb = b >> 5;   // bits 31 + lo .. hi belong to all 32 windows
    uint32_t mid = row[ka] & (0xffffffffu << (a & 31));
    if (ka == kb) mid &= 0xffffffffu >> (31 - (b & 31));
    else {
        for (int k = ka + 1; k < kb; ++k) mid |= row[k];
        mid |= row[kb] & (0xffffffffu >> (31 - (b & 31)));
    }
    return head | tail | (mid ? 0xffffffffu : 0u);
}
MK_HD inline uint32_t mk_morph_out(const MkJob& J, int w, uint32_t acc) {
    return ((J.flags & kMkCompOut) ? ~acc : acc) & mk_colmask(J.W, w);
}
constexpr int kMkBand = kMkStageRows - kMkTileR + 1;     // element rows one staged band serves

// A workgroup's tile (32 dwords from w0, 32 rows from y0), one band [i0, i1) of element rows at a time; lane = 0 .. 255.  The kernel and
// the host check both run these three per lane, the kernel with barriers between them.
struct MkAcc { uint32_t r0, r8, r16, r24; };             // a lane's output dwords: column lane & 31, rows lane / 32 + 0, 8, 16, 24
MK_HD inline int mk_band_end(const MkJob& J, int i0) { return i0 + kMkBand < J.kh ? i0 + kMkBand : J.kh; }
// staged dwords of the band: 32 + (i1 - i0) - 1 rows (at most kMkStageRows) of 32 + 2 halo dwords
MK_HD inline int mk_band_dwords(const MkJob& J, int i0) { return (kMkTileR + mk_band_end(J, i0) - i0 - 1) * (kMkTileW + 2 * J.halo); }
MK_HD inline void mk_morph_stage(const MkJob& J, int y0, int w0, int i0, int lane, uint32_t* stage) {
    const int n = mk_band_dwords(J, i0), sw = kMkTileW + 2 * J.halo;
    for (int idx = lane; idx < n; idx += kMkThreads) stage[idx] = mk_stage_word(J, y0, w0, i0 - J.ay, sw, idx);
}
MK_HD inline void mk_morph_band(const MkJob& J, int w0, int i0, int lane, const uint32_t* stage, MkAcc& acc) {
    const int wx = lane & (kMkTileW - 1), ry = lane / kMkTileW, sw = kMkTileW + 2 * J.halo, wl = wx + J.halo, i1 = mk_band_end(J, i0);
    if (w0 + wx >= J.pw) return;
    for (int i = i0; i < i1; ++i) {
        int dy, lo, hi;
        if (!mk_span(J, i, &dy, &lo, &hi)) continue;
        const uint32_t* row = stage + (ry + dy - (i0 - J.ay)) * sw;
        acc.r0 |= mk_row_or(row, wl, lo, hi);
        acc.r8 |= mk_row_or(row + 8 * sw, wl, lo, hi);
        acc.r16 |= mk_row_or(row + 16 * sw, wl, lo, hi);
        acc.r24 |= mk_row_or(row + 24 * sw, wl, lo, hi);
    }
}
MK_HD inline void mk_morph_store(const MkJob& J, int y0, int w0, int lane, const MkAcc& acc) {
    const int w = w0 + (lane & (kMkTileW - 1)), y = y0 + lane / kMkTileW;
    if (w >= J.pw) return;
    uint32_t* out = J.out + (int64_t)y * J.pw + w;
    if (y < J.H) out[0] = mk_morph_out(J, w, acc.r0);
    if (y + 8 < J.H) out[8 * (int64_t)J.pw] = mk_morph_out(J, w, acc.r8);
    if (y + 16 < J.H) out[16 * (int64_t)J.pw] = mk_morph_out(J, w, acc.r16);
    if (y + 24 < J.H) out[24 * (int64_t)J.pw] = mk_morph_out(J, w, acc.r24);
}

// ---- fuse ------------------------------------------------------------------------------------------------------------------------
// item q of a job's fills (mk_fuse_items); integer atomic ORs, which commute
MK_HD inline void mk_fuse_item(const MkJob& J, int q) {
    const int pw = J.pw, H = J.H, W = J.W, f = J.f, s = J.s;
    if (q < 2 * pw) {                                     // rows 0 .. y_min (top) or y_max .. H - 1 (bottom) of every column with a set row
        const bool top = q < pw;
        const int w = top ? q : q - pw, ya = top ? 0 : H - f, step = top ? 1 : -1, y_first = top ? ya : H - 1;
        uint32_t any = 0;
        for (int k = 0; k < f; ++k) any |= J.in[(int64_t)(ya + k) * pw + w];
        if (!any) return;
        uint32_t seen = 0;
        for (int k = 0, y = y_first; k < f; ++k, y += step) {
            const uint32_t cur = J.in[(int64_t)y * pw + w], fill = any & ~seen & ~cur;
            if (fill) mk_atomic_or(J.out + (int64_t)y * pw + w, fill);
            seen |= cur;
        }
        return;
    }
    q -= 2 * pw;
    const bool left = q < H;
    const int y = left ? q : q - H;
    const int r0 = y - s < 0 ? 0 : y - s, r1 = y + s > H - 1 ? H - 1 : y + s;     // the seeds spread s rows up and down
    const int x0 = left ? 0 : W - f, x1 = left ? f : W;                           // the strip's columns [x0, x1)
    const int wa = x0 >> 5, wb = (x1 - 1) >> 5;
    for (int k = 0; k <= wb - wa; ++k) {                  // towards the inside: the first dword with a seed holds x_min (x_max)
        const int w = left ? wa + k : wb - k;
        uint32_t m = mk_colmask(x1, w);
        if (w == wa) m &= 0xffffffffu << (x0 & 31);
        uint32_t v = 0;
        for (int r = r0; r <= r1; ++r) v |= J.in[(int64_t)r * pw + w];
        v &= m;
        if (!v) continue;
        uint32_t* row = J.out + (int64_t)y * pw;
        if (left) {
            for (int u = 0; u < w; ++u) mk_atomic_or(row + u, 0xffffffffu);
            mk_atomic_or(row + w, 0xffffffffu >> (31 - mk_ctz(v)));
        } else {
            mk_atomic_or(row + w, (0xffffffffu << (31 - mk_clz(v))) & mk_colmask(W, w));
            for (int u = w + 1; u < pw; ++u) mk_atomic_or(row + u, mk_colmask(W, u));
        }
        return;
    }
}

// ---- finish ----------------------------------------------------------------------------------------------------------------------
// pixel (y, x) of the output; count: the mask's set pixels (zero takes the reference's `mask is None` branches)
MK_HD inline void mk_compose(const MkJob& J, int y, int x, uint32_t count) {
    const bool m = mk_bit(J.out, J.pw, y, x);
    const uint8_t on = J.invert ? 0 : 255, off = J.invert ? 255 : 0;
    if (J.kind == GS360_MASK_OUT_MASK) {
        J.dst[(int64_t)y * J.dst_stride + x] = m ? on : off;
        return;
    }
    const uint8_t* px = J.img + (int64_t)y * J.img_stride + 3 * (int64_t)x;
    const uint8_t r = px[0], g = px[1], b = px[2];
    if (J.kind == GS360_MASK_OUT_RGBA) {
        uint8_t* o = J.dst + (int64_t)y * J.dst_stride + 4 * (int64_t)x;
        o[0] = r; o[1] = g; o[2] = b;
        o[3] = count ? (m ? on : off) : 0;
        return;
    }
    const bool keep = !count || (J.kind == GS360_MASK_OUT_KEEP ? m : !m);
    uint8_t* o = J.dst + (int64_t)y * J.dst_stride + 3 * (int64_t)x;
    o[0] = keep ? r : 0; o[1] = keep ? g : 0; o[2] = keep ? b : 0;
}

// GS360_MASK_OUT_MASK, four pixels from column x (a multiple of 4) on
MK_HD inline void mk_compose_mask4(const MkJob& J, int y, int x) {
    if (x >= J.W) return;
    const uint32_t nib = mk_plane_nibble(J.out, J.pw, y, x), on = J.invert ? 0u : 255u, off = 255u - on;
    uint32_t v = 0;
    for (int k = 0; k < 4; ++k) v |= (((nib >> k) & 1u) ? on : off) << (8 * k);
    mk_store4(J.dst + (int64_t)y * J.dst_stride + x, x, J.W, v);
}

__global__ void __launch_bounds__(kMkThreads) mk_pack_kernel(const MkLaunch L) {
    const MkJob& J = L.job[job_of(L, blockIdx.x, &MkJob::tile_base)];
    int y, tx;
    mk_tile_of(J, &y, &tx);
    const int x = tx * kMkPackTile.w + 4 * threadIdx.x;
    mk_store_word(J.out, J.pw, y, x, mk_gather8(mk_nibble(J.src, J.src_stride, J.W, J.thresh, y, x)));
}

__global__ void __launch_bounds__(kMkThreads) mk_morph_kernel(const MkLaunch L) {
    __shared__ uint32_t stage[kMkStageRows * kMkStageW];
    const MkJob& J = L.job[job_of(L, blockIdx.x, &MkJob::tile_base)];
    int ty, tx;
    mk_tile_of(J, &ty, &tx);
    const int w0 = tx * kMkMorphTile.w, y0 = ty * kMkMorphTile.h;
    MkAcc acc = {0, 0, 0, 0};
    for (int i0 = 0; i0 < J.kh; i0 += kMkBand) {
        __syncthreads();
        mk_morph_stage(J, y0, w0, i0, threadIdx.x, stage);
        __syncthreads();
        mk_morph_band(J, w0, i0, threadIdx.x, stage, acc);
    }
    mk_morph_store(J, y0, w0, threadIdx.x, acc);
}

__global__ void __launch_bounds__(kMkThreads) mk_fuse_kernel(const MkLaunch L) {
    const MkJob& J = L.job[job_of(L, blockIdx.x, &MkJob::tile_base)];
    const int64_t q = mk_item_of(J);
    if (L.phase == 0) {
        if (q < mk_plane_items(J)) J.out[q] = J.in[q];
    } else if (q < mk_fuse_items(J)) {
        mk_fuse_item(J, (int)q);
    }
}

__global__ void __launch_bounds__(kMkThreads) mk_finish_kernel(const MkLaunch L) {
    const int j = job_of(L, blockIdx.x, &MkJob::tile_base);
    const MkJob& J = L.job[j];
    int y, tx;
    mk_tile_of(J, &y, &tx);
    if (L.phase == 1) {                                   // the mask: four pixels per lane; the compose kinds: one
        const int lane = tx * kMkThreads + threadIdx.x;   // mk_output_tile: mk_output_px pixels for each of the row's lanes
        if (J.kind == GS360_MASK_OUT_MASK) mk_compose_mask4(J, y, mk_output_px(GS360_MASK_OUT_MASK) * lane);
        else if (lane < J.W) mk_compose(J, y, lane, L.counts[j]);
        return;
    }
    // phase 0: four pixels per lane and a band of rows per workgroup
    const int x = tx * kMkCountTile.w + 4 * threadIdx.x, y1 = min(J.H, (y + 1) * kMkCountTile.h);
    uint32_t n = 0;
    for (y *= kMkCountTile.h; y < y1; ++y) {
        const uint32_t nib = mk_plane_nibble(J.out, J.pw, y, x) | mk_nibble(J.add, J.add_stride, J.W, 0, y, x);
        if (J.add) mk_store_word(J.out, J.pw, y, x, mk_gather8(nib));   // (the shuffles wait for the eight lanes' reads of the dword)
        n += (uint32_t)__popc(nib);
    }
    mk_count_tail(n, L.counts + j);
}

}  // namespace

hipError_t launch_mask_pack_bits(const MkLaunch& L, hipStream_t s) { return mk_launch(mk_pack_kernel, L, s); }
hipError_t launch_mask_morph(const MkLaunch& L, hipStream_t s) { return mk_launch(mk_morph_kernel, L, s); }
hipError_t launch_mask_fuse(const MkLaunch& L, hipStream_t s) { return mk_launch(mk_fuse_kernel, L, s); }
hipError_t launch_mask_finish(const MkLaunch& L, hipStream_t s) { return mk_launch(mk_finish_kernel, L, s); }

}  // namespace gs360
