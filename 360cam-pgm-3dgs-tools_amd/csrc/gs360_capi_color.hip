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

struct gs360_color_plan16 {
    int device = 0;
    gs360::Color16Launch L;
    float* d_lut = nullptr;
    float* d_thr = nullptr;
    void* d_bins = nullptr;
};

// what both creates check first
static int check_create(gs360_ctx* c, bool have_args, int lut_size) {
    if (!c) return fail(GS360_ERR_ARG, "ctx is NULL");
    if (!have_args) return fail(GS360_ERR_ARG, "NULL argument");
    if (lut_size < 2 || lut_size > 256) return fail(GS360_ERR_ARG, "LUT size %d outside [2,256]", lut_size);
    return GS360_OK;
}

// Release a plan's device memory and the plan itself (create's failure path and destroy); the first hipFree error, if any.
template <typename Plan>
static hipError_t release_plan(Plan* p, std::initializer_list<void*> mem) {
    hipError_t e = hipSuccess;
    for (void* d : mem)
        if (d) { const hipError_t f = hipFree(d); if (e == hipSuccess) e = f; }
    delete p;
    return e;
}
static hipError_t release_plan(gs360_color_plan* p) { return release_plan(p, {p->d_rtab, p->d_tables, p->d_cube}); }
static hipError_t release_plan(gs360_color_plan16* p) { return release_plan(p, {p->d_lut, p->d_thr, p->d_bins}); }

template <typename Plan>
static int destroy_plan(gs360_ctx* c, Plan* p) {
    if (!c) return fail(GS360_ERR_ARG, "ctx is NULL");
    if (!p) return GS360_OK;
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(release_plan(p));
    return GS360_OK;
}

// What both apply calls check, for samples of `bytes` bytes.  Fills the image record, default strides included; an empty image is
// GS360_OK with the record left without a source.
static int check_apply(gs360_ctx* c, const int* plan_device, const void* src, int H, int W, int C, size_t src_stride, int red_index,
                       void* dst, size_t dst_stride, int slot, int bytes, ColorImage& I) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    if (!plan_device || !src || !dst) return fail(GS360_ERR_ARG, "NULL argument");
    if (*plan_device != c->device) return fail(GS360_ERR_ARG, "colour plan belongs to device %d, ctx is device %d", *plan_device, c->device);
    if (C != 3 && C != 4) return fail(GS360_ERR_ARG, "the LUT stage needs 3 or 4 channels (got %d)", C);   // DF:693-697
    if (red_index != 0 && red_index != 2) return fail(GS360_ERR_ARG, "red_index must be 0 (RGB) or 2 (BGR)");
    if (H < 0 || W < 0) return fail(GS360_ERR_ARG, "bad size");
    if (H == 0 || W == 0) return GS360_OK;
    if (H > 65535) return fail(GS360_ERR_UNSUPPORTED, "image height %d above 65535", H);
    const size_t row = (size_t)W * C * bytes;
    if (src_stride == 0) src_stride = row;
    if (dst_stride == 0) dst_stride = row;
    const bool short_row = src_stride < row || dst_stride < row;
    if (bytes == 1 && short_row) return fail(GS360_ERR_ARG, "stride smaller than a row");
    if (bytes == 2 && (short_row || ((src_stride | dst_stride) & 1))) return fail(GS360_ERR_ARG, "16-bit images need even strides of at least one row");
    HIP_TRY(hipSetDevice(c->device));
    I = ColorImage{src, dst, H, W, red_index, (int64_t)src_stride, (int64_t)dst_stride};
    return GS360_OK;
}

int gs360_color_plan_create(gs360_ctx* c, const float* lut, int lut_size, const float* level_pos,
                            const float* out_thresholds, gs360_color_plan** out) {
    if (int rc = check_create(c, lut && level_pos && out_thresholds && out, lut_size)) return rc;
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
        (void)release_plan(p);
        return fail(e == hipErrorOutOfMemory ? GS360_ERR_NOMEM : GS360_ERR_HIP, "colour plan setup failed: %s", hipGetErrorString(e));
    }
    *out = p;
    return GS360_OK;
}

int gs360_color_plan_destroy(gs360_ctx* c, gs360_color_plan* p) { return destroy_plan(c, p); }

int gs360_color_apply_u8(gs360_ctx* c, const gs360_color_plan* p, const void* src, int H, int W, int C, size_t src_stride,
                         int red_index, void* dst, size_t dst_stride, int slot) {
    ColorLaunch L{};
    if (int rc = check_apply(c, p ? &p->device : nullptr, src, H, W, C, src_stride, red_index, dst, dst_stride, slot, 1, L.img)) return rc;
    if (!L.img.src) return GS360_OK;
    L.rtab = p->d_rtab; L.tables = p->d_tables; L.cube = p->d_cube; L.lut_size = p->lut_size; L.fixups = p->fixups;
    HIP_TRY(launch_color(L, C, c->stream[slot]));
    return GS360_OK;
}

int gs360_color_plan16_create(gs360_ctx* c, const float* lut, int lut_size, const float* domain_min, const float* domain_max,
                              int n_pieces, const float* piece_start, const int32_t* piece_base, const int32_t* piece_off,
                              const float* thresholds, gs360_color_plan16** out) {
    if (int rc = check_create(c, lut && domain_min && domain_max && out, lut_size)) return rc;
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
        (void)release_plan(p);
        return fail(GS360_ERR_HIP, "colour plan setup failed: %s", hipGetErrorString(e));
    }
    p->L.lut = p->d_lut;
    p->L.thr = p->d_thr;
    p->L.bins = p->d_bins;
    *out = p;
    return GS360_OK;
}

int gs360_color_plan16_destroy(gs360_ctx* c, gs360_color_plan16* p) { return destroy_plan(c, p); }

int gs360_color_apply_u16(gs360_ctx* c, const gs360_color_plan16* p, const void* src, int H, int W, int C, size_t src_stride,
                          int red_index, void* dst, size_t dst_stride, int slot) {
    ColorImage I{};
    if (int rc = check_apply(c, p ? &p->device : nullptr, src, H, W, C, src_stride, red_index, dst, dst_stride, slot, 2, I)) return rc;
    if (!I.src) return GS360_OK;
    gs360::Color16Launch L = p->L;
    L.img = I;
    HIP_TRY(launch_color16(L, C, c->stream[slot]));
    return GS360_OK;
}
