// gs360_capi_framescore.hip -- C-ABI glue of the frame sharpness statistics, edge score, FFT energy and optical flow
// (include/gs360.h; kernels in gs360_framescore.hip, gs360_framefft.hip and gs360_frameflow.hip).
#include "gs360_capi_internal.h"

using namespace gs360;

namespace {

int check_frame_size(int H, int W) {
    if (H <= 0 || W <= 0) return fail(GS360_ERR_ARG, "bad size %d x %d", W, H);
    if (H > 65535 || W > 65535) return fail(GS360_ERR_UNSUPPORTED, "frame %d x %d above 65535 on a side", W, H);
    return 0;
}

// A source frame of `depth` bits per sample (8 or 16): channels, channel order and size, then the row stride in bytes (0 = packed
// rows, filled in here)
int check_frame_layout(int H, int W, int C, int depth, int red_index, size_t* stride) {
    if (int rc = check_channels(C)) return rc;
    if (red_index != 0 && red_index != 2) return fail(GS360_ERR_ARG, "red_index must be 0 (RGB) or 2 (BGR)");
    if (int rc = check_frame_size(H, W)) return rc;
    const size_t row = (size_t)W * C * (depth / 8);
    if (*stride == 0) *stride = row;
    if (*stride < row) return fail(GS360_ERR_ARG, "stride smaller than a row");
    return 0;
}

// FS-DEPTH16 v1's size bound: every pixel can add (8 * 65535)^2 to sum_lap2 (columns of 0 and 65535 in turn; sum_mag2's largest
// term, 2 * (4 * 65535)^2, is smaller), and the sums are signed 64-bit.
static_assert(GS360_FS16_MAX_PIXELS == INT64_MAX / ((int64_t)(8 * 65535) * (8 * 65535)), "GS360_FS16_MAX_PIXELS");
int check_stats_pixels(int H, int W, int depth) {
    if (depth == 16 && (int64_t)H * W > GS360_FS16_MAX_PIXELS)
        return fail(GS360_ERR_UNSUPPORTED, "16-bit frame %d x %d above %lld pixels: its sums of squares could pass 64 bits", W, H,
                    (long long)GS360_FS16_MAX_PIXELS);
    return 0;
}

int check_band(int band_y0, int band_y1, int H) {
    if (band_y0 < 0 || band_y1 > H || band_y0 >= band_y1) return fail(GS360_ERR_ARG, "band [%d,%d) outside [0,%d) or empty", band_y0, band_y1, H);
    return 0;
}

// The frame pointers of a call: none NULL, each 4-byte aligned (the kernels stage rows with dword loads)
int check_frame_pointers(const void* const* frames, int n_frames) {
    for (int f = 0; f < n_frames; ++f) {
        if (!frames[f]) return fail(GS360_ERR_ARG, "frames[%d] is NULL", f);
        if ((uintptr_t)frames[f] & 3) return fail(GS360_ERR_ARG, "frames[%d] is not 4-byte aligned", f);
    }
    return 0;
}

// cv::resize: inv_scale = dsize / ssize, scale = 1 / inv_scale (both INTER_AREA's tables and INTER_NEAREST's index)
double cv_resize_scale(int dsize, int ssize) { return 1.0 / ((double)dsize / ssize); }

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// FS-FLOW's resize path: 0 none, 1 INTER_AREA integer factors (cv::resize's is_area_fast), 2 the general area tables
int flow_resize_mode(int cw, int ch, int sw, int sh, int* kx, int* ky) {
    if (sw == cw && sh == ch) return 0;
    const double sx = cv_resize_scale(sw, cw), sy = cv_resize_scale(sh, ch);
    const int ix = (int)std::nearbyint(sx), iy = (int)std::nearbyint(sy);
    if (std::fabs(sx - ix) < 2.220446049250313e-16 && std::fabs(sy - iy) < 2.220446049250313e-16 && sw * ix == cw && sh * iy == ch) {
        *kx = ix; *ky = iy;
        return 1;
    }
    return 2;
}

// gs360_frame_stats_u8 / _u16: one body, `depth` bits per sample
int frame_stats(gs360_ctx* c, const void* const* frames, int n_frames, int H, int W, int C, int depth, size_t stride, int red_index,
                int band_y0, int band_y1, uint32_t flags, gs360_frame_stats* stats_dev, float* const* small_dev, int small_w,
                int small_h, int slot) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    if (n_frames < 0) return fail(GS360_ERR_ARG, "n_frames < 0");
    if (n_frames == 0) return GS360_OK;
    if (!frames || !stats_dev) return fail(GS360_ERR_ARG, "NULL argument");
    if (int rc = check_frame_layout(H, W, C, depth, red_index, &stride)) return rc;
    if (int rc = check_stats_pixels(H, W, depth)) return rc;
    if (int rc = check_band(band_y0, band_y1, H)) return rc;
    if (flags & ~(GS360_FS_CIRCLE | GS360_FS_HIGHLIGHTS)) return fail(GS360_ERR_ARG, "unknown flags 0x%x", flags);
    if (int rc = check_frame_pointers(frames, n_frames)) return rc;
    for (int f = 0; small_dev && f < n_frames; ++f)
        if (!small_dev[f]) return fail(GS360_ERR_ARG, "small_dev[%d] is NULL", f);
    if (small_dev && (small_w < 1 || small_w > W || small_h < 1 || small_h > band_y1 - band_y0))
        return fail(GS360_ERR_ARG, "small image %d x %d outside [1,%d] x [1,%d]", small_w, small_h, W, band_y1 - band_y0);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream[slot];
    HIP_TRY(hipMemsetAsync(stats_dev, 0, (size_t)n_frames * sizeof(gs360_frame_stats), s));
    FsLaunch L;
    std::memset(&L, 0, sizeof(L));
    L.stride = (int64_t)stride;
    L.H = H; L.W = W; L.C = C; L.red = red_index; L.depth = depth;
    L.y0 = band_y0; L.y1 = band_y1;
    L.circle = (flags & GS360_FS_CIRCLE) ? 1 : 0;
    L.highlights = (flags & GS360_FS_HIGHLIGHTS) ? 1 : 0;
    if (small_dev) {
        L.small_w = small_w; L.small_h = small_h;
        L.scale_x = cv_resize_scale(small_w, W);
        L.scale_y = cv_resize_scale(small_h, band_y1 - band_y0);
    }
    for (int f0 = 0; f0 < n_frames; f0 += GS360_MAX_FRAMES) {
        L.n_frames = std::min(GS360_MAX_FRAMES, n_frames - f0);
        for (int k = 0; k < L.n_frames; ++k) {
            L.src[k] = (const uint8_t*)frames[f0 + k];
            L.small[k] = small_dev ? small_dev[f0 + k] : nullptr;
        }
        L.stats = stats_dev + f0;
        HIP_TRY(launch_frame_stats(L, s));
    }
    return GS360_OK;
}

// gs360_frame_edge_u8 / _u16
int frame_edge(gs360_ctx* c, const void* const* frames, int n_frames, int H, int W, int C, int depth, size_t stride, int red_index,
               int band_y0, int band_y1, gs360_frame_edge* out_dev, int slot) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    if (n_frames < 0) return fail(GS360_ERR_ARG, "n_frames < 0");
    if (n_frames == 0) return GS360_OK;
    if (!frames || !out_dev) return fail(GS360_ERR_ARG, "NULL argument");
    if (int rc = check_frame_layout(H, W, C, depth, red_index, &stride)) return rc;
    if (int rc = check_band(band_y0, band_y1, H)) return rc;
    if (int rc = check_frame_pointers(frames, n_frames)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream[slot];
    HIP_TRY(hipMemsetAsync(out_dev, 0, (size_t)n_frames * sizeof(gs360_frame_edge), s));
    FsLaunch L;
    std::memset(&L, 0, sizeof(L));
    L.stride = (int64_t)stride;
    L.H = H; L.W = W; L.C = C; L.red = red_index; L.depth = depth;
    L.y0 = band_y0; L.y1 = band_y1;
    for (int f0 = 0; f0 < n_frames; f0 += GS360_MAX_FRAMES) {
        L.n_frames = std::min(GS360_MAX_FRAMES, n_frames - f0);
        for (int k = 0; k < L.n_frames; ++k) L.src[k] = (const uint8_t*)frames[f0 + k];
        L.edge = out_dev + f0;
        HIP_TRY(launch_frame_edge(L, s));
    }
    return GS360_OK;
}

}  // namespace

int gs360_frame_stats_u8(gs360_ctx* c, const void* const* frames, int n_frames, int H, int W, int C, size_t stride, int red_index,
                         int band_y0, int band_y1, uint32_t flags, gs360_frame_stats* stats_dev, float* const* small_dev, int small_w,
                         int small_h, int slot) {
    return frame_stats(c, frames, n_frames, H, W, C, 8, stride, red_index, band_y0, band_y1, flags, stats_dev, small_dev, small_w,
                       small_h, slot);
}

int gs360_frame_stats_u16(gs360_ctx* c, const void* const* frames, int n_frames, int H, int W, int C, size_t stride, int red_index,
                          int band_y0, int band_y1, uint32_t flags, gs360_frame_stats* stats_dev, float* const* small_dev, int small_w,
                          int small_h, int slot) {
    return frame_stats(c, frames, n_frames, H, W, C, 16, stride, red_index, band_y0, band_y1, flags, stats_dev, small_dev, small_w,
                       small_h, slot);
}

int gs360_frame_edge_u8(gs360_ctx* c, const void* const* frames, int n_frames, int H, int W, int C, size_t stride, int red_index,
                        int band_y0, int band_y1, gs360_frame_edge* out_dev, int slot) {
    return frame_edge(c, frames, n_frames, H, W, C, 8, stride, red_index, band_y0, band_y1, out_dev, slot);
}

int gs360_frame_edge_u16(gs360_ctx* c, const void* const* frames, int n_frames, int H, int W, int C, size_t stride, int red_index,
                         int band_y0, int band_y1, gs360_frame_edge* out_dev, int slot) {
    return frame_edge(c, frames, n_frames, H, W, C, 16, stride, red_index, band_y0, band_y1, out_dev, slot);
}

int gs360_frame_fft_energy(gs360_ctx* c, const float* const* small_dev, int n_frames, int small_w, int small_h, int H, int W,
                           int band_y0, int band_y1, uint32_t flags, gs360_frame_fft* out_dev, int slot) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    if (n_frames < 0) return fail(GS360_ERR_ARG, "n_frames < 0");
    if (n_frames == 0) return GS360_OK;
    if (!small_dev || !out_dev) return fail(GS360_ERR_ARG, "NULL argument");
    if (int rc = check_frame_size(H, W)) return rc;
    if (int rc = check_band(band_y0, band_y1, H)) return rc;
    if (flags & ~(GS360_FS_CIRCLE | GS360_FS_HIGHLIGHTS)) return fail(GS360_ERR_ARG, "unknown flags 0x%x", flags);
    const int bh = band_y1 - band_y0;
    if (small_w < 1 || small_w > std::min(W, GS360_FFT_MAX_SIDE) || small_h < 1 || small_h > std::min(bh, GS360_FFT_MAX_SIDE))
        return fail(GS360_ERR_ARG, "fft input %d x %d outside [1,%d] x [1,%d]", small_w, small_h, std::min(W, GS360_FFT_MAX_SIDE),
                    std::min(bh, GS360_FFT_MAX_SIDE));
    for (int f = 0; f < n_frames; ++f)
        if (!small_dev[f]) return fail(GS360_ERR_ARG, "small_dev[%d] is NULL", f);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream[slot];
    FfLaunch L;
    std::memset(&L, 0, sizeof(L));
    L.h = small_h; L.w = small_w; L.K = small_w / 2 + 1;
    L.n_part = frame_fft_partials(small_h, small_w);
    L.H = H; L.W = W; L.y0 = band_y0; L.y1 = band_y1;
    L.circle = (flags & GS360_FS_CIRCLE) ? 1 : 0;
    L.highlights = (flags & GS360_FS_HIGHLIGHTS) ? 1 : 0;
    L.scale_x = cv_resize_scale(small_w, W);      // INTER_NEAREST, as gs360_frame_stats_u8's nearest plane
    L.scale_y = cv_resize_scale(small_h, bh);
    // per-slot workspace for one launch: the partials, then each frame's row-pass spectrum (2 x h x K float32)
    const size_t part_bytes = (size_t)GS360_MAX_FRAMES * L.n_part * sizeof(FfPartial);
    const size_t x_bytes = (size_t)2 * L.h * L.K * sizeof(float);
    Staging& st = c->stage[slot];
    if (int rc = ensure(&st.d_fft, &st.fft_cap, part_bytes + (size_t)GS360_MAX_FRAMES * x_bytes)) return rc;
    L.part = (FfPartial*)st.d_fft;
    for (int k = 0; k < GS360_MAX_FRAMES; ++k) L.x[k] = (float*)((uint8_t*)st.d_fft + part_bytes + x_bytes * k);
    for (int f0 = 0; f0 < n_frames; f0 += GS360_MAX_FRAMES) {
        L.n_frames = std::min(GS360_MAX_FRAMES, n_frames - f0);
        for (int k = 0; k < L.n_frames; ++k) L.small[k] = small_dev[f0 + k];
        L.out = out_dev + f0;
        HIP_TRY(launch_frame_fft(L, s));
    }
    return GS360_OK;
}

namespace {

// gs360_frame_flow_u8 / _u16
int frame_flow(gs360_ctx* c, const void* const* frames, int n_frames, int H, int W, int C, int depth, size_t stride, int red_index,
               int crop_x0, int crop_y0, int crop_w, int crop_h, int small_w, int small_h, uint32_t flags, const int* pairs,
               int n_pairs, gs360_frame_flow* out_dev, gs360_flow_point* points_dev, int slot) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    if (n_pairs < 0 || n_frames < 0) return fail(GS360_ERR_ARG, "n_frames or n_pairs < 0");
    if (n_pairs == 0) return GS360_OK;
    if (!frames || !pairs || !out_dev) return fail(GS360_ERR_ARG, "NULL argument");
    if (int rc = check_frame_layout(H, W, C, depth, red_index, &stride)) return rc;
    if (crop_w < 1 || crop_h < 1 || crop_x0 < 0 || crop_y0 < 0 || crop_x0 + crop_w > W || crop_y0 + crop_h > H)
        return fail(GS360_ERR_ARG, "crop %d x %d at (%d, %d) outside the %d x %d frame", crop_w, crop_h, crop_x0, crop_y0, W, H);
    if (small_w < 1 || small_h < 1 || small_w > std::min(crop_w, GS360_FLOW_MAX_SIDE) || small_h > std::min(crop_h, GS360_FLOW_MAX_SIDE))
        return fail(GS360_ERR_ARG, "small image %d x %d outside [1,%d] x [1,%d]", small_w, small_h, std::min(crop_w, GS360_FLOW_MAX_SIDE),
                    std::min(crop_h, GS360_FLOW_MAX_SIDE));
    if (flags & ~GS360_FS_CIRCLE) return fail(GS360_ERR_ARG, "unknown flags 0x%x", flags);
    for (int k = 0; k < 2 * n_pairs; ++k) {
        if (pairs[k] < 0 || pairs[k] >= n_frames) return fail(GS360_ERR_ARG, "pairs[%d] = %d outside [0,%d)", k, pairs[k], n_frames);
        if (!frames[pairs[k]]) return fail(GS360_ERR_ARG, "frames[%d] is NULL", pairs[k]);
    }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream[slot];

    FlLaunch L;
    std::memset(&L, 0, sizeof(L));
    L.stride = (int64_t)stride;
    L.H = H; L.W = W; L.C = C; L.red = red_index; L.depth = depth;
    L.circle = (flags & GS360_FS_CIRCLE) ? 1 : 0;
    L.cx0 = crop_x0; L.cy0 = crop_y0; L.cw = crop_w; L.ch = crop_h; L.sw = small_w; L.sh = small_h;
    L.mode = flow_resize_mode(crop_w, crop_h, small_w, small_h, &L.kx, &L.ky);
    L.scale_x = cv_resize_scale(small_w, crop_w);
    L.scale_y = cv_resize_scale(small_h, crop_h);
    // buildOpticalFlowPyramid(winSize 15, maxLevel 2): the next level's ((w+1)/2, (h+1)/2) must exceed 15 on both sides
    int w = small_w, h = small_h;
    L.levels = 0;
    for (int lev = 0; lev < 3; ++lev) {
        L.lw[lev] = w; L.lh[lev] = h; L.pitch[lev] = w + 30;
        L.levels = lev + 1;
        w = (w + 1) / 2; h = (h + 1) / 2;
        if (w <= 15 || h <= 15) break;
    }
    size_t off = 0;
    for (int lev = 0; lev < L.levels; ++lev) {
        const size_t px = (size_t)L.pitch[lev] * (L.lh[lev] + 30);
        L.img_off[lev] = off; off = align256(off + px);
        L.der_off[lev] = off; off = align256(off + 4 * px);
    }
    L.corner_off = off; off = align256(off + (size_t)GS360_FLOW_MAX_CORNERS * 8);
    L.ncorner_off = off; off = align256(off + 4);
    L.state_bytes = off;
    const size_t npx = (size_t)small_w * small_h;
    const size_t ncand = (small_w >= 3 && small_h >= 3) ? (size_t)(small_w - 2) * (small_h - 2) : 1;
    L.key_cap = 2048;
    while ((size_t)L.key_cap < ncand) L.key_cap <<= 1;
    off = 0;
    L.mask_off = off; off = align256(off + npx);
    L.sob_off = off; off = align256(off + 4 * npx);
    L.eig_off = off; off = align256(off + 4 * npx);
    L.cnt_off = off; off += 256;
    L.key_off = off; off = align256(off + 8 * (size_t)L.key_cap);
    L.work_bytes = off;
    const size_t state_all = (size_t)kFlSlots * L.state_bytes, work_all = (size_t)GS360_MAX_FRAMES * L.work_bytes;
    const size_t pts_all = (size_t)kFlMaxPairs * GS360_FLOW_MAX_CORNERS * sizeof(gs360_flow_point);
    Staging& st = c->stage[slot];
    if (int rc = ensure(&st.d_flow, &st.flow_cap, state_all + work_all + pts_all)) return rc;
    L.state = (uint8_t*)st.d_flow;
    L.work = L.state + state_all;
    FlPairs Q;
    std::memset(&Q, 0, sizeof(Q));
    Q.points = (gs360_flow_point*)(L.work + work_all);
    Q.user_points = points_dev;
    Q.out = out_dev;

    // Pairs in order, in groups whose frames fit one batch; a frame already resident from the previous group is not recomputed.
    std::vector<int> slot_of(n_frames, -1), owner(kFlSlots, -1);
    for (int p = 0; p < n_pairs;) {
        std::vector<int> fr;
        int q = p;
        while (q < n_pairs && q - p < kFlMaxPairs) {
            std::vector<int> t = fr;
            for (int e = 0; e < 2; ++e)
                if (std::find(t.begin(), t.end(), pairs[2 * q + e]) == t.end()) t.push_back(pairs[2 * q + e]);
            if ((int)t.size() > GS360_MAX_FRAMES) break;
            fr.swap(t);
            ++q;
        }
        std::vector<bool> keep(kFlSlots, false);
        for (int f : fr)
            if (slot_of[f] >= 0) keep[slot_of[f]] = true;
        L.n_frames = 0;
        int free_slot = 0;
        for (int f : fr) {
            if (slot_of[f] >= 0) continue;
            while (keep[free_slot]) ++free_slot;   // <= 16 kept, <= 16 new: a free slot always exists among 32
            if (owner[free_slot] >= 0) slot_of[owner[free_slot]] = -1;
            owner[free_slot] = f;
            slot_of[f] = free_slot;
            keep[free_slot] = true;
            L.src[L.n_frames] = (const uint8_t*)frames[f];
            L.slot[L.n_frames] = free_slot;
            ++L.n_frames;
        }
        if (L.n_frames) {
            HIP_TRY(hipMemset2DAsync(L.work + L.cnt_off, L.work_bytes, 0, L.work_bytes - L.cnt_off, L.n_frames, s));
            HIP_TRY(launch_frame_flow_frames(L, s));
        }
        Q.n_pairs = q - p;
        for (int k = 0; k < Q.n_pairs; ++k) {
            Q.prev[k] = slot_of[pairs[2 * (p + k)]];
            Q.curr[k] = slot_of[pairs[2 * (p + k) + 1]];
            Q.out_index[k] = p + k;
        }
        HIP_TRY(launch_frame_flow_pairs(L, Q, s));
        p = q;
    }
    return GS360_OK;
}

}  // namespace

int gs360_frame_flow_u8(gs360_ctx* c, const void* const* frames, int n_frames, int H, int W, int C, size_t stride, int red_index,
                        int crop_x0, int crop_y0, int crop_w, int crop_h, int small_w, int small_h, uint32_t flags, const int* pairs,
                        int n_pairs, gs360_frame_flow* out_dev, gs360_flow_point* points_dev, int slot) {
    return frame_flow(c, frames, n_frames, H, W, C, 8, stride, red_index, crop_x0, crop_y0, crop_w, crop_h, small_w, small_h, flags,
                      pairs, n_pairs, out_dev, points_dev, slot);
}

int gs360_frame_flow_u16(gs360_ctx* c, const void* const* frames, int n_frames, int H, int W, int C, size_t stride, int red_index,
                         int crop_x0, int crop_y0, int crop_w, int crop_h, int small_w, int small_h, uint32_t flags, const int* pairs,
                         int n_pairs, gs360_frame_flow* out_dev, gs360_flow_point* points_dev, int slot) {
    return frame_flow(c, frames, n_frames, H, W, C, 16, stride, red_index, crop_x0, crop_y0, crop_w, crop_h, small_w, small_h, flags,
                      pairs, n_pairs, out_dev, points_dev, slot);
}
