// gs360_capi_mask.hip -- the mask-finishing entry points of libgs360hip.so (include/gs360.h; MSK-SPEC v1):
// validation, the scratch layout and the launch sequence of the kernels in gs360_maskmorph.hip.
#include "gs360_capi_internal.h"

using namespace gs360;

namespace {

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline size_t plane_bytes(const gs360_mask_job& j) { return round_up((size_t)j.H * ((size_t)(j.W + 31) / 32) * 4, 256); }
inline size_t rows_bytes(int kh) { return round_up((size_t)kh * 8, 256); }

// the largest |column offset| an element reaches, or -1 for a span outside the element
int element_reach(const int32_t* rows, int kw, int kh) {
    int reach = 0;
    for (int i = 0; i < kh; ++i) {
        const int j1 = rows[2 * i], j2 = rows[2 * i + 1];
        if (j1 < 0 || j2 < j1 || j2 > kw) return -1;
        if (j2 > j1) reach = std::max({reach, std::abs(j1 - kw / 2), std::abs(j2 - 1 - kw / 2)});
    }
    return reach;
}

int check_element(int k, const char* name, int kw, int kh, const int32_t* rows) {
    if (kh == 0) return 0;
    if (kw < 1 || kh < 1) return fail(GS360_ERR_ARG, "job %d: %s element of %d x %d", k, name, kw, kh);
    if (kw > GS360_MASK_MAX_ELEMENT || kh > GS360_MASK_MAX_ELEMENT)
        return fail(GS360_ERR_UNSUPPORTED, "job %d: %s element of %d x %d above %d", k, name, kw, kh, GS360_MASK_MAX_ELEMENT);
    if (!rows) return fail(GS360_ERR_ARG, "job %d: %s element without rows", k, name);
    if (element_reach(rows, kw, kh) < 0) return fail(GS360_ERR_ARG, "job %d: %s element has a span outside its %d columns", k, name, kw);
    return 0;
}

int check_job(int k, const gs360_mask_job& j) {
    if (j.H < 1 || j.W < 1) return fail(GS360_ERR_ARG, "job %d: mask of %d x %d", k, j.W, j.H);
    if (j.H > GS360_MASK_MAX_SIDE || j.W > GS360_MASK_MAX_SIDE)
        return fail(GS360_ERR_UNSUPPORTED, "job %d: mask sides are 1..%d (got %d x %d)", k, GS360_MASK_MAX_SIDE, j.W, j.H);
    if (j.kind < GS360_MASK_OUT_MASK || j.kind > GS360_MASK_OUT_REMOVE) return fail(GS360_ERR_ARG, "job %d: unknown output kind %d", k, j.kind);
    if (!j.dst) return fail(GS360_ERR_ARG, "job %d: NULL output", k);
    if (j.kind != GS360_MASK_OUT_MASK && !j.image) return fail(GS360_ERR_ARG, "job %d: output kind %d needs the image", k, j.kind);
    const size_t out_c = j.kind == GS360_MASK_OUT_MASK ? 1 : j.kind == GS360_MASK_OUT_RGBA ? 4 : 3;
    if ((j.src_stride && j.src_stride < (size_t)j.W) || (j.add_stride && j.add_stride < (size_t)j.W) ||
        (j.image_stride && j.image_stride < (size_t)j.W * 3) || (j.dst_stride && j.dst_stride < (size_t)j.W * out_c))
        return fail(GS360_ERR_ARG, "job %d: a stride below a row", k);
    if (j.thresh < 0 || j.thresh > 255) return fail(GS360_ERR_ARG, "job %d: thresh %d outside 0..255", k, j.thresh);
    if (int rc = check_element(k, "close", j.close_kw, j.close_kh, j.close_rows)) return rc;
    if (int rc = check_element(k, "expand", j.expand_kw, j.expand_kh, j.expand_rows)) return rc;
    if (j.fuse < 0 || j.fuse > std::min(j.H, j.W)) return fail(GS360_ERR_ARG, "job %d: fuse %d outside 0..min(H, W)", k, j.fuse);
    if (j.spread < 0) return fail(GS360_ERR_ARG, "job %d: spread %d", k, j.spread);
    // a lane of the side strips reads (2 spread + 1) rows of fuse / 32 dwords
    if (j.fuse > GS360_MASK_MAX_FUSE || (j.fuse > 0 && j.spread > GS360_MASK_MAX_FUSE))
        return fail(GS360_ERR_UNSUPPORTED, "job %d: fuse %d / spread %d above %d", k, j.fuse, j.spread, GS360_MASK_MAX_FUSE);
    return 0;
}

// a batch's scratch: per job two planes, then its close and expand rows
size_t batch_bytes(const gs360_mask_job* jobs, int n) {
    size_t b = 0;
    for (int k = 0; k < n; ++k) b += 2 * plane_bytes(jobs[k]) + rows_bytes(jobs[k].close_kh) + rows_bytes(jobs[k].expand_kh);
    return b;
}

int check_jobs(const gs360_mask_job* jobs, int n_jobs, size_t* need) {
    if (n_jobs < 0) return fail(GS360_ERR_ARG, "n_jobs < 0");
    if (n_jobs && !jobs) return fail(GS360_ERR_ARG, "NULL argument");
    *need = 0;
    for (int k = 0; k < n_jobs; ++k)
        if (int rc = check_job(k, jobs[k])) return rc;
    for (int k0 = 0; k0 < n_jobs; k0 += GS360_MAX_VIEWS) *need = std::max(*need, batch_bytes(jobs + k0, std::min(GS360_MAX_VIEWS, n_jobs - k0)));
    return 0;
}

// row tiles of a job: workgroups of `px` pixels by `rows` rows
int64_t row_tiles(MkJob& J, int px, int rows) {
    J.tiles_x = (J.W + px - 1) / px;
    return (int64_t)J.tiles_x * ((J.H + rows - 1) / rows);
}

// one step over the batch: `tiles_of(k, J)` sets the step's fields of job k and returns its tiles (0: the job skips the step); the
// jobs' tiles are numbered in job order
template <class Tiles>
int run_step(MkLaunch& L, hipError_t (*launch)(const MkLaunch&, hipStream_t), hipStream_t s, Tiles tiles_of) {
    int64_t tiles = 0;
    for (int k = 0; k < L.n_jobs; ++k) {
        MkJob& J = L.job[k];
        J.tile_base = (int32_t)tiles;
        J.tiles_x = 1;
        tiles += tiles_of(k, J);
        if (tiles > INT32_MAX) return fail(GS360_ERR_ARG, "mask batch too large");
    }
    L.total_tiles = (int32_t)tiles;
    HIP_TRY(launch(L, s));
    return 0;
}

}  // namespace

int gs360_mask_finish_scratch(const gs360_mask_job* jobs, int n_jobs, size_t* bytes) {
    if (!bytes) return fail(GS360_ERR_ARG, "NULL argument");
    size_t need = 0;
    if (int rc = check_jobs(jobs, n_jobs, &need)) return rc;
    *bytes = need;
    return GS360_OK;
}

int gs360_mask_finish_u8(gs360_ctx* c, const gs360_mask_job* jobs, int n_jobs, void* scratch_dev, size_t scratch_bytes,
                         uint32_t* counts_dev, int slot) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    size_t need = 0;
    if (int rc = check_jobs(jobs, n_jobs, &need)) return rc;
    if (n_jobs == 0) return GS360_OK;
    if (!scratch_dev || !counts_dev) return fail(GS360_ERR_ARG, "NULL argument");
    if ((uintptr_t)scratch_dev % 256) return fail(GS360_ERR_ARG, "scratch is not 256-byte aligned");
    if (scratch_bytes < need) return fail(GS360_ERR_ARG, "scratch of %zu bytes below the %zu the jobs need", scratch_bytes, need);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream[slot];
    HIP_TRY(hipMemsetAsync(counts_dev, 0, (size_t)n_jobs * sizeof(uint32_t), s));
    for (int k0 = 0; k0 < n_jobs; k0 += GS360_MAX_VIEWS) {
        MkLaunch L;
        std::memset(&L, 0, sizeof(L));
        L.n_jobs = std::min(GS360_MAX_VIEWS, n_jobs - k0);
        L.counts = counts_dev + k0;
        uint32_t* plane[GS360_MAX_VIEWS][2];
        const int32_t* spans[GS360_MAX_VIEWS][2];
        int halo[GS360_MAX_VIEWS][2], cur[GS360_MAX_VIEWS] = {};
        uint8_t* at = (uint8_t*)scratch_dev;
        for (int k = 0; k < L.n_jobs; ++k) {
            const gs360_mask_job& j = jobs[k0 + k];
            MkJob& J = L.job[k];
            J.src = (const uint8_t*)j.src; J.add = (const uint8_t*)j.add; J.img = (const uint8_t*)j.image; J.dst = (uint8_t*)j.dst;
            const int out_c = j.kind == GS360_MASK_OUT_MASK ? 1 : j.kind == GS360_MASK_OUT_RGBA ? 4 : 3;
            J.src_stride = (int64_t)(j.src_stride ? j.src_stride : (size_t)j.W);
            J.add_stride = (int64_t)(j.add_stride ? j.add_stride : (size_t)j.W);
            J.img_stride = (int64_t)(j.image_stride ? j.image_stride : (size_t)j.W * 3);
            J.dst_stride = (int64_t)(j.dst_stride ? j.dst_stride : (size_t)j.W * out_c);
            J.H = j.H; J.W = j.W; J.pw = (j.W + 31) / 32; J.thresh = j.thresh;
            J.f = j.fuse; J.s = j.spread; J.kind = j.kind; J.invert = j.invert != 0;
            plane[k][0] = (uint32_t*)at; at += plane_bytes(j);
            plane[k][1] = (uint32_t*)at; at += plane_bytes(j);
            const int kh[2] = {j.close_kh, j.expand_kh}, kw[2] = {j.close_kw, j.expand_kw};
            const int32_t* host[2] = {j.close_rows, j.expand_rows};
            for (int e = 0; e < 2; ++e) {
                spans[k][e] = (const int32_t*)at;
                halo[k][e] = kh[e] ? element_reach(host[e], kw[e], kh[e]) / 32 + 2 : 0;   // at most kMkMaxHalo: check_element bounds kw
                if (kh[e]) HIP_TRY(hipMemcpyAsync(at, host[e], (size_t)kh[e] * 8, hipMemcpyHostToDevice, s));
                at += rows_bytes(kh[e]);
            }
        }
        HIP_TRY(hipStreamSynchronize(s));                 // the caller's element rows are read; the earlier batch is done with the scratch
        auto flip = [&](int k, MkJob& J) { J.in = plane[k][cur[k]]; J.out = plane[k][cur[k] ^ 1]; };
        auto morph = [&](int e, int flags) {              // element e (0 close, 1 expand) over the jobs that have one
            int rc = run_step(L, launch_mask_morph, s, [&](int k, MkJob& J) -> int64_t {
                const gs360_mask_job& j = jobs[k0 + k];
                const int kh = e ? j.expand_kh : j.close_kh, kw = e ? j.expand_kw : j.close_kw;
                if (!kh) return 0;
                flip(k, J);
                J.spans = spans[k][e]; J.kh = kh; J.ax = kw / 2; J.ay = kh / 2; J.halo = halo[k][e]; J.flags = flags;
                J.tiles_x = (J.pw + kMkTileW - 1) / kMkTileW;
                return (int64_t)J.tiles_x * ((J.H + kMkTileR - 1) / kMkTileR);
            });
            for (int k = 0; k < L.n_jobs; ++k) cur[k] ^= (e ? jobs[k0 + k].expand_kh : jobs[k0 + k].close_kh) != 0;
            return rc;
        };
        if (int rc = run_step(L, launch_mask_pack_bits, s, [&](int k, MkJob& J) { J.out = plane[k][0]; return row_tiles(J, 4 * kMkThreads, 1); })) return rc;
        if (int rc = morph(0, 0)) return rc;                                  // close: dilate ...
        if (int rc = morph(0, kMkCompIn | kMkCompOut)) return rc;             // ... then erode
        if (int rc = morph(1, 0)) return rc;                                  // expand
        for (int phase = 0; phase < 2; ++phase) {                             // edge fuse: copy, then the fills
            L.phase = phase;
            if (int rc = run_step(L, launch_mask_fuse, s, [&](int k, MkJob& J) -> int64_t {
                    if (!J.f) return 0;
                    flip(k, J);
                    const int64_t items = phase ? 2 * (int64_t)J.pw + 2 * (int64_t)J.H : (int64_t)J.H * J.pw;
                    return (items + kMkThreads - 1) / kMkThreads;
                })) return rc;
        }
        for (int k = 0; k < L.n_jobs; ++k) cur[k] ^= L.job[k].f != 0;
        for (int phase = 0; phase < 2; ++phase) {                             // add layer and count, then the output
            L.phase = phase;
            if (int rc = run_step(L, launch_mask_finish, s, [&](int k, MkJob& J) {
                    J.out = plane[k][cur[k]];
                    if (!phase) return row_tiles(J, 4 * kMkThreads, kMkFinishRows);
                    return row_tiles(J, J.kind == GS360_MASK_OUT_MASK ? 4 * kMkThreads : kMkThreads, 1);
                })) return rc;
        }
    }
    return GS360_OK;
}
