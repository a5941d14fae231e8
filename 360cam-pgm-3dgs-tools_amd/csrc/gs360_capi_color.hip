// gs360_capi_color.hip -- C-ABI glue of the input colour stage (include/gs360.h): 8- and 16-bit colour plans and their apply calls.
#include "gs360_capi_internal.h"

using namespace gs360;

struct gs360_color_plan {
    int device = 0;
    int lut_size = 0;
    int fixups = 0;
    void* d_rtab = nullptr;     // cell-major red-interpolated LUT, see gs360_color.hip (released once the cube is built)
    float* d_tables = nullptr;  // level positions, thresholds, bin levels
    void* d_cube = nullptr;     // uint32[2^24]: the stage evaluated for every 8-bit pixel (NULL with GS360_COLOR_CUBE=0)
};

int gs360_color_plan_create(gs360_ctx* c, const float* lut, int lut_size, const float* level_pos,
                            const float* out_thresholds, gs360_color_plan** out) {
    if (!c) return fail(GS360_ERR_ARG, "ctx is NULL");
    if (!lut || !level_pos || !out_thresholds || !out) return fail(GS360_ERR_ARG, "NULL argument");
    if (lut_size < 2 || lut_size > 256) return fail(GS360_ERR_ARG, "LUT size %d outside [2,256]", lut_size);
    const int nmax = lut_size - 1;
    for (int i = 0; i < 768; ++i)   // positions index the table: refuse anything that would read outside it
        if (!(level_pos[i] >= 0.0f && level_pos[i] <= (float)nmax))
            return fail(GS360_ERR_ARG, "level_pos[%d] = %g outside [0,%d]", i, (double)level_pos[i], nmax);
    for (int k = 1; k < 256; ++k) {
        if (!(out_thresholds[k] >= 0.0f)) return fail(GS360_ERR_ARG, "out_thresholds[%d] is negative or NaN", k);
        if (k > 1 && !(out_thresholds[k] >= out_thresholds[k - 1]))
            return fail(GS360_ERR_ARG, "out_thresholds must be non-decreasing (entry %d)", k);
    }
    HIP_TRY(hipSetDevice(c->device));
    gs360_color_plan* p = new (std::nothrow) gs360_color_plan();
    if (!p) return fail(GS360_ERR_NOMEM, "out of host memory");
    p->device = c->device;
    p->lut_size = lut_size;
    const size_t n3 = (size_t)lut_size * lut_size * lut_size;
    std::vector<float> tables(color_tables_floats(), 0.0f);
    std::memcpy(tables.data(), level_pos, 768 * sizeof(float));
    std::memcpy(tables.data() + 768, out_thresholds, 256 * sizeof(float));
    p->fixups = color_build_bins(out_thresholds, (uint8_t*)(tables.data() + 1024));
    float* d_lut = nullptr;
    hipError_t e = hipMalloc((void**)&d_lut, n3 * 3 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&p->d_rtab, color_rtab_bytes(lut_size) + kSlack);
    if (e == hipSuccess) e = hipMalloc((void**)&p->d_tables, tables.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(d_lut, lut, n3 * 3 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p->d_tables, tables.data(), tables.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = build_color_rtab(d_lut, p->d_tables /* red positions come first */, p->d_rtab, lut_size, c->stream[0]);
    const bool want_cube = opt(c, kOptColorCube) != 0;      // option "color_cube" (-1 / 1: yes)
    if (e == hipSuccess && want_cube) {
        e = hipMalloc(&p->d_cube, color_cube_bytes());
        if (e == hipErrorOutOfMemory) {          // a crowded device: the per-pixel evaluation gives the same results from the 18 MB it already has
            (void)hipGetLastError();
            p->d_cube = nullptr;
            e = hipSuccess;
        } else if (e == hipSuccess) {
            ColorLaunch B{};
            B.rtab = p->d_rtab; B.tables = p->d_tables; B.lut_size = lut_size; B.fixups = p->fixups;
            e = build_color_cube(B, p->d_cube, c->stream[0]);
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream[0]);
    if (d_lut) (void)hipFree(d_lut);
    if (e == hipSuccess && p->d_cube) {          // the cube replaces the tables it was built from
        (void)hipFree(p->d_rtab);
        p->d_rtab = nullptr;
    }
    if (e != hipSuccess) {
        if (p->d_rtab) (void)hipFree(p->d_rtab);
        if (p->d_tables) (void)hipFree(p->d_tables);
        if (p->d_cube) (void)hipFree(p->d_cube);
        delete p;
        return fail(e == hipErrorOutOfMemory ? GS360_ERR_NOMEM : GS360_ERR_HIP, "colour plan setup failed: %s", hipGetErrorString(e));
    }
    *out = p;
    return GS360_OK;
}

int gs360_color_plan_destroy(gs360_ctx* c, gs360_color_plan* p) {
    if (!c) return fail(GS360_ERR_ARG, "ctx is NULL");
    if (!p) return GS360_OK;
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipDeviceSynchronize());
    if (p->d_rtab) HIP_TRY(hipFree(p->d_rtab));
    if (p->d_tables) HIP_TRY(hipFree(p->d_tables));
    if (p->d_cube) HIP_TRY(hipFree(p->d_cube));
    delete p;
    return GS360_OK;
}

int gs360_color_apply_u8(gs360_ctx* c, const gs360_color_plan* p, const void* src, int H, int W, int C, size_t src_stride,
                         int red_index, void* dst, size_t dst_stride, int slot) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    if (!p || !src || !dst) return fail(GS360_ERR_ARG, "NULL argument");
    if (p->device != c->device) return fail(GS360_ERR_ARG, "colour plan belongs to device %d, ctx is device %d", p->device, c->device);
    if (C != 3 && C != 4) return fail(GS360_ERR_ARG, "the LUT stage needs 3 or 4 channels (got %d)", C);   // DF:693-697
    if (red_index != 0 && red_index != 2) return fail(GS360_ERR_ARG, "red_index must be 0 (RGB) or 2 (BGR)");
    if (H < 0 || W < 0) return fail(GS360_ERR_ARG, "bad size");
    if (H == 0 || W == 0) return GS360_OK;
    if (H > 65535) return fail(GS360_ERR_UNSUPPORTED, "image height %d above 65535", H);
    if (src_stride == 0) src_stride = (size_t)W * C;
    if (dst_stride == 0) dst_stride = (size_t)W * C;
    if (src_stride < (size_t)W * C || dst_stride < (size_t)W * C) return fail(GS360_ERR_ARG, "stride smaller than a row");
    HIP_TRY(hipSetDevice(c->device));
    ColorLaunch L;
    L.src = (const uint8_t*)src; L.dst = (uint8_t*)dst; L.rtab = p->d_rtab; L.tables = p->d_tables; L.cube = p->d_cube;
    L.H = H; L.W = W; L.lut_size = p->lut_size; L.red_index = red_index; L.fixups = p->fixups;
    L.src_stride = (int64_t)src_stride; L.dst_stride = (int64_t)dst_stride;
    HIP_TRY(launch_color(L, C, c->stream[slot]));
    return GS360_OK;
}

struct gs360_color_plan16 {
    int device = 0;
    gs360::Color16Launch L;
    float* d_lut = nullptr;
    float* d_thr = nullptr;
    void* d_bins = nullptr;
};

int gs360_color_plan16_create(gs360_ctx* c, const float* lut, int lut_size, const float* domain_min, const float* domain_max,
                              int n_pieces, const float* piece_start, const int32_t* piece_base, const int32_t* piece_off,
                              const float* thresholds, gs360_color_plan16** out) {
    if (!c) return fail(GS360_ERR_ARG, "ctx is NULL");
    if (!lut || !domain_min || !domain_max || !out) return fail(GS360_ERR_ARG, "NULL argument");
    if (lut_size < 2 || lut_size > 256) return fail(GS360_ERR_ARG, "LUT size %d outside [2,256]", lut_size);
    if (n_pieces < 0 || n_pieces > 4) return fail(GS360_ERR_ARG, "n_pieces must be in [0,4]");
    if (n_pieces && (!piece_start || !piece_base || !piece_off || !thresholds)) return fail(GS360_ERR_ARG, "NULL piece tables");
    gs360_color_plan16* p = new (std::nothrow) gs360_color_plan16();
    if (!p) return fail(GS360_ERR_NOMEM, "out of host memory");
    std::memset(&p->L, 0, sizeof(p->L));
    for (int k = 0; k < 3; ++k) {
        p->L.dmin[k] = domain_min[k];
        p->L.span[k] = domain_max[k] - domain_min[k];                 // float32 subtraction, DF:641
        if (!(p->L.span[k] > 0.0f)) { delete p; return fail(GS360_ERR_ARG, "invalid LUT domain on channel %d", k); }
    }
    int total = 0;
    for (int q = 0; q < n_pieces; ++q) {
        const int lo = piece_off[q], hi = piece_off[q + 1];
        if (lo != total || hi < lo || hi > (1 << 20)) { delete p; return fail(GS360_ERR_ARG, "piece_off must be contiguous and ascending"); }
        for (int i = lo + 1; i < hi; ++i)
            if (!(thresholds[i] >= thresholds[i - 1])) { delete p; return fail(GS360_ERR_ARG, "thresholds of piece %d are not sorted (entry %d)", q, i); }
        if (piece_base[q] < 0 || piece_base[q] + (hi - lo) > 65535) { delete p; return fail(GS360_ERR_ARG, "piece %d would produce levels above 65535", q); }
        if (q > 0 && !(piece_start[q] >= piece_start[q - 1])) { delete p; return fail(GS360_ERR_ARG, "piece_start must be ascending"); }
        p->L.start[q] = q ? piece_start[q] : 0.0f;
        p->L.base[q] = piece_base[q];
        p->L.off[q] = lo;
        total = hi;
    }
    p->L.off[n_pieces] = total;
    p->L.n_pieces = n_pieces;
    p->L.lut_size = lut_size;
    p->device = c->device;
    const size_t n3 = (size_t)lut_size * lut_size * lut_size * 3;
    hipError_t e = hipSetDevice(c->device);                     // (a failure here must release the host plan too)
    if (e == hipSuccess) e = hipMalloc((void**)&p->d_lut, n3 * sizeof(float) + kSlack);
    if (e == hipSuccess) e = hipMemcpy(p->d_lut, lut, n3 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess && total) e = hipMalloc((void**)&p->d_thr, (size_t)total * sizeof(float));
    if (e == hipSuccess && total) e = hipMemcpy(p->d_thr, thresholds, (size_t)total * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess && n_pieces) {
        std::vector<uint8_t> bins(color16_bins_bytes());
        color16_build_bins(n_pieces, p->L.start, p->L.off, thresholds, bins.data());
        e = hipMalloc((void**)&p->d_bins, bins.size());
        if (e == hipSuccess) e = hipMemcpy(p->d_bins, bins.data(), bins.size(), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        if (p->d_lut) (void)hipFree(p->d_lut);
        if (p->d_thr) (void)hipFree(p->d_thr);
        if (p->d_bins) (void)hipFree(p->d_bins);
        delete p;
        return fail(GS360_ERR_HIP, "colour plan setup failed: %s", hipGetErrorString(e));
    }
    p->L.lut = p->d_lut;
    p->L.thr = p->d_thr;
    p->L.bins = p->d_bins;
    *out = p;
    return GS360_OK;
}

int gs360_color_plan16_destroy(gs360_ctx* c, gs360_color_plan16* p) {
    if (!c) return fail(GS360_ERR_ARG, "ctx is NULL");
    if (!p) return GS360_OK;
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipDeviceSynchronize());
    if (p->d_lut) HIP_TRY(hipFree(p->d_lut));
    if (p->d_thr) HIP_TRY(hipFree(p->d_thr));
    if (p->d_bins) HIP_TRY(hipFree(p->d_bins));
    delete p;
    return GS360_OK;
}

int gs360_color_apply_u16(gs360_ctx* c, const gs360_color_plan16* p, const void* src, int H, int W, int C, size_t src_stride,
                          int red_index, void* dst, size_t dst_stride, int slot) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    if (!p || !src || !dst) return fail(GS360_ERR_ARG, "NULL argument");
    if (p->device != c->device) return fail(GS360_ERR_ARG, "colour plan belongs to device %d, ctx is device %d", p->device, c->device);
    if (C != 3 && C != 4) return fail(GS360_ERR_ARG, "the LUT stage needs 3 or 4 channels (got %d)", C);
    if (red_index != 0 && red_index != 2) return fail(GS360_ERR_ARG, "red_index must be 0 (RGB) or 2 (BGR)");
    if (H < 0 || W < 0) return fail(GS360_ERR_ARG, "bad size");
    if (H == 0 || W == 0) return GS360_OK;
    if (H > 65535) return fail(GS360_ERR_UNSUPPORTED, "image height %d above 65535", H);
    if (src_stride == 0) src_stride = (size_t)W * C * 2;
    if (dst_stride == 0) dst_stride = (size_t)W * C * 2;
    if (src_stride < (size_t)W * C * 2 || dst_stride < (size_t)W * C * 2 || ((src_stride | dst_stride) & 1))
        return fail(GS360_ERR_ARG, "16-bit images need even strides of at least one row");
    HIP_TRY(hipSetDevice(c->device));
    gs360::Color16Launch L = p->L;
    L.src = src; L.dst = dst; L.H = H; L.W = W; L.red_index = red_index;
    L.src_stride = (int64_t)src_stride; L.dst_stride = (int64_t)dst_stride;
    HIP_TRY(launch_color16(L, C, c->stream[slot]));
    return GS360_OK;
}
