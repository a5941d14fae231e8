// gs360_capi_framescore.hip -- C-ABI glue of the frame sharpness statistics and the frame FFT energy (include/gs360.h; kernels in
// gs360_framescore.hip and gs360_framefft.hip).
#include "gs360_capi_internal.h"

using namespace gs360;

int gs360_frame_stats_u8(gs360_ctx* c, const void* const* frames, int n_frames, int H, int W, int C, size_t stride, int red_index,
                         int band_y0, int band_y1, uint32_t flags, gs360_frame_stats* stats_dev, float* const* small_dev, int small_w,
                         int small_h, int slot) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    if (n_frames < 0) return fail(GS360_ERR_ARG, "n_frames < 0");
    if (n_frames == 0) return GS360_OK;
    if (!frames || !stats_dev) return fail(GS360_ERR_ARG, "NULL argument");
    if (int rc = check_channels(C)) return rc;
    if (red_index != 0 && red_index != 2) return fail(GS360_ERR_ARG, "red_index must be 0 (RGB) or 2 (BGR)");
    if (H <= 0 || W <= 0) return fail(GS360_ERR_ARG, "bad size %d x %d", W, H);
    if (H > 65535 || W > 65535) return fail(GS360_ERR_UNSUPPORTED, "frame %d x %d above 65535 on a side", W, H);
    if (stride == 0) stride = (size_t)W * C;
    if (stride < (size_t)W * C) return fail(GS360_ERR_ARG, "stride smaller than a row");
    if (band_y0 < 0 || band_y1 > H || band_y0 >= band_y1) return fail(GS360_ERR_ARG, "band [%d,%d) outside [0,%d) or empty", band_y0, band_y1, H);
    if (flags & ~(GS360_FS_CIRCLE | GS360_FS_HIGHLIGHTS)) return fail(GS360_ERR_ARG, "unknown flags 0x%x", flags);
    for (int f = 0; f < n_frames; ++f) {
        if (!frames[f]) return fail(GS360_ERR_ARG, "frames[%d] is NULL", f);
        if ((uintptr_t)frames[f] & 3) return fail(GS360_ERR_ARG, "frames[%d] is not 4-byte aligned", f);   // dword row loads
        if (small_dev && !small_dev[f]) return fail(GS360_ERR_ARG, "small_dev[%d] is NULL", f);
    }
    if (small_dev && (small_w < 1 || small_w > W || small_h < 1 || small_h > band_y1 - band_y0))
        return fail(GS360_ERR_ARG, "small image %d x %d outside [1,%d] x [1,%d]", small_w, small_h, W, band_y1 - band_y0);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream[slot];
    HIP_TRY(hipMemsetAsync(stats_dev, 0, (size_t)n_frames * sizeof(gs360_frame_stats), s));
    FsLaunch L;
    std::memset(&L, 0, sizeof(L));
    L.stride = (int64_t)stride;
    L.H = H; L.W = W; L.C = C; L.red = red_index;
    L.y0 = band_y0; L.y1 = band_y1;
    L.circle = (flags & GS360_FS_CIRCLE) ? 1 : 0;
    L.highlights = (flags & GS360_FS_HIGHLIGHTS) ? 1 : 0;
    if (small_dev) {   // cv::resize: inv_scale = dsize / ssize, scale = 1 / inv_scale (both INTER_AREA's tables and INTER_NEAREST's index)
        L.small_w = small_w; L.small_h = small_h;
        L.scale_x = 1.0 / ((double)small_w / W);
        L.scale_y = 1.0 / ((double)small_h / (band_y1 - band_y0));
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

int gs360_frame_fft_energy(gs360_ctx* c, const float* const* small_dev, int n_frames, int small_w, int small_h, int H, int W,
                           int band_y0, int band_y1, uint32_t flags, gs360_frame_fft* out_dev, int slot) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    if (n_frames < 0) return fail(GS360_ERR_ARG, "n_frames < 0");
    if (n_frames == 0) return GS360_OK;
    if (!small_dev || !out_dev) return fail(GS360_ERR_ARG, "NULL argument");
    if (H <= 0 || W <= 0) return fail(GS360_ERR_ARG, "bad size %d x %d", W, H);
    if (H > 65535 || W > 65535) return fail(GS360_ERR_UNSUPPORTED, "frame %d x %d above 65535 on a side", W, H);
    if (band_y0 < 0 || band_y1 > H || band_y0 >= band_y1) return fail(GS360_ERR_ARG, "band [%d,%d) outside [0,%d) or empty", band_y0, band_y1, H);
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
    L.scale_x = 1.0 / ((double)small_w / W);      // cv::resize INTER_NEAREST, as gs360_frame_stats_u8's nearest plane
    L.scale_y = 1.0 / ((double)small_h / bh);
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
