// gs360_capi_mask.hip -- the mask-finishing entry points of libgs360hip.so (include/gs360.h; MSK-SPEC v1, MSK-SHADOW v1 and MSK-INPAINT
// v1): validation, the scratch layout and the launch sequence of the kernels in gs360_maskmorph.hip,
// gs360_maskshadow.hip and gs360_maskinpaint.hip.
// Every grid is sized by the function of gs360_maskplane.h that bounds its kernel.
#include "gs360_capi_internal.h"
#include "gs360_maskplane.h"

using namespace gs360;

namespace {

inline size_t plane_bytes(int H, int W) { return round_up((size_t)H * ((size_t)(W + 31) / 32) * 4, 256); }
inline size_t plane_bytes(const gs360_mask_job& j) { return plane_bytes(j.H, j.W); }
inline size_t rows_bytes(int kh) { return round_up((size_t)kh * 8, 256); }
inline int64_t stride_or(size_t stride, size_t row) { return (int64_t)(stride ? stride : row); }
inline int out_channels(int kind) { return kind == GS360_MASK_OUT_MASK ? 1 : kind == GS360_MASK_OUT_RGBA ? 4 : 3; }

int check_element(int k, const char* name, int kw, int kh, const int32_t* rows) {
    if (kh == 0) return 0;
    if (kw < 1 || kh < 1) return fail(GS360_ERR_ARG, "job %d: %s element of %d x %d", k, name, kw, kh);
    if (kw > GS360_MASK_MAX_ELEMENT || kh > GS360_MASK_MAX_ELEMENT)
        return fail(GS360_ERR_UNSUPPORTED, "job %d: %s element of %d x %d above %d", k, name, kw, kh, GS360_MASK_MAX_ELEMENT);
    if (!rows) return fail(GS360_ERR_ARG, "job %d: %s element without rows", k, name);
    if (mk_element_halo(rows, kw, kh) < 0) return fail(GS360_ERR_ARG, "job %d: %s element has a span outside its %d columns", k, name, kw);
    return 0;
}

// a checked element of a job as the morph kernel takes it (a job without it has kh == 0); its rows are staged at `dev`
struct Element {
    int kw, kh, halo;                    // halo: at most kMkMaxHalo, check_element bounds kw
    const int32_t* rows;                 // device memory
};
Element element_of(int kw, int kh, const int32_t* rows, const void* dev) { return {kw, kh, mk_element_halo(rows, kw, kh), (const int32_t*)dev}; }
int stage_rows(void* dev, const int32_t* rows, int kh, hipStream_t s) {
    if (kh) HIP_TRY(hipMemcpyAsync(dev, rows, (size_t)kh * 8, hipMemcpyHostToDevice, s));
    return 0;
}

int check_job(int k, const gs360_mask_job& j) {
    if (j.H < 1 || j.W < 1) return fail(GS360_ERR_ARG, "job %d: mask of %d x %d", k, j.W, j.H);
    if (j.H > GS360_MASK_MAX_SIDE || j.W > GS360_MASK_MAX_SIDE)
        return fail(GS360_ERR_UNSUPPORTED, "job %d: mask sides are 1..%d (got %d x %d)", k, GS360_MASK_MAX_SIDE, j.W, j.H);
    if (j.kind < GS360_MASK_OUT_MASK || j.kind > GS360_MASK_OUT_REMOVE) return fail(GS360_ERR_ARG, "job %d: unknown output kind %d", k, j.kind);
    if (!j.dst) return fail(GS360_ERR_ARG, "job %d: NULL output", k);
    if (j.kind != GS360_MASK_OUT_MASK && !j.image) return fail(GS360_ERR_ARG, "job %d: output kind %d needs the image", k, j.kind);
    if ((j.src_stride && j.src_stride < (size_t)j.W) || (j.add_stride && j.add_stride < (size_t)j.W) ||
        (j.image_stride && j.image_stride < (size_t)j.W * 3) || (j.dst_stride && j.dst_stride < (size_t)j.W * out_channels(j.kind)))
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

// what every call with jobs in it does between its jobs' checks, which gave `need`, and its first copy: the buffers' checks, the
// slot's stream, the counts cleared
int begin_call(gs360_ctx* c, int slot, int n_jobs, const void* scratch_dev, size_t scratch_bytes, size_t need, uint32_t* counts_dev,
               hipStream_t* s) {
    if (!scratch_dev || !counts_dev) return fail(GS360_ERR_ARG, "NULL argument");
    if ((uintptr_t)scratch_dev % 256) return fail(GS360_ERR_ARG, "scratch is not 256-byte aligned");
    if (scratch_bytes < need) return fail(GS360_ERR_ARG, "scratch of %zu bytes below the %zu the jobs need", scratch_bytes, need);
    HIP_TRY(hipSetDevice(c->device));
    *s = c->stream[slot];
    HIP_TRY(hipMemsetAsync(counts_dev, 0, (size_t)n_jobs * sizeof(uint32_t), *s));
    return 0;
}

// row tiles of a job: workgroups of t.w pixels by t.h rows
template <class Job>
int64_t row_tiles(Job& J, MkTile t) { return mk_tiles(J, J.W, t); }

// one step over the batch: `tiles_of(k, J)` sets the step's fields of job k and returns its tiles (0: the job skips the step); the
// jobs' tiles are numbered in job order
template <class Launch, class Fn, class Tiles>
int run_step(Launch& L, Fn launch, hipStream_t s, Tiles tiles_of) {
    int64_t tiles = 0;
    for (int k = 0; k < L.n_jobs; ++k) {
        auto& J = L.job[k];
        J.tile_base = (int32_t)tiles;
        J.tiles_x = 1;
        tiles += tiles_of(k, J);
        if (tiles > INT32_MAX) return fail(GS360_ERR_ARG, "mask batch too large");
    }
    L.total_tiles = (int32_t)tiles;
    HIP_TRY(launch(L, s));
    return 0;
}

// one dilate or erode over the batch: plane from(k) -> plane to(k) by el[k]; a job without the element skips the step
template <class From, class To>
int morph_step(MkLaunch& L, hipStream_t s, From from, To to, const Element* el, int flags) {
    return run_step(L, launch_mask_morph, s, [&](int k, MkJob& J) -> int64_t {
        const Element& e = el[k];
        if (!e.kh) return 0;
        J.in = from(k); J.out = to(k);
        J.spans = e.rows; J.kh = e.kh; J.ax = e.kw / 2; J.ay = e.kh / 2; J.halo = e.halo; J.flags = flags;
        return mk_tiles(J, J.pw, kMkMorphTile);
    });
}

// the jobs [k0, k0 + n) of a finishing call as one launch: two planes per job, the one that holds the mask so far is cur[k]
struct FinishBatch {
    MkLaunch mk;
    uint32_t* plane[GS360_MAX_VIEWS][2];
    int cur[GS360_MAX_VIEWS];
    Element close[GS360_MAX_VIEWS], expand[GS360_MAX_VIEWS];
    uint32_t* held(int k) const { return plane[k][cur[k]]; }
    uint32_t* other(int k) const { return plane[k][cur[k] ^ 1]; }
};
int finish_batch(FinishBatch& B, const gs360_mask_job* jobs, int n, uint8_t* at, uint32_t* counts, hipStream_t s) {
    std::memset(&B.mk, 0, sizeof(B.mk));
    B.mk.n_jobs = n;
    B.mk.counts = counts;
    for (int k = 0; k < n; ++k) {
        const gs360_mask_job& j = jobs[k];
        MkJob& J = B.mk.job[k];
        J.src = (const uint8_t*)j.src; J.add = (const uint8_t*)j.add; J.img = (const uint8_t*)j.image; J.dst = (uint8_t*)j.dst;
        J.src_stride = stride_or(j.src_stride, (size_t)j.W);
        J.add_stride = stride_or(j.add_stride, (size_t)j.W);
        J.img_stride = stride_or(j.image_stride, (size_t)j.W * 3);
        J.dst_stride = stride_or(j.dst_stride, (size_t)j.W * out_channels(j.kind));
        J.H = j.H; J.W = j.W; J.pw = (j.W + 31) / 32; J.thresh = j.thresh;
        J.f = j.fuse; J.s = j.spread; J.kind = j.kind; J.invert = j.invert != 0;
        B.cur[k] = 0;
        B.plane[k][0] = (uint32_t*)at; at += plane_bytes(j);
        B.plane[k][1] = (uint32_t*)at; at += plane_bytes(j);
        B.close[k] = element_of(j.close_kw, j.close_kh, j.close_rows, at);
        if (int rc = stage_rows(at, j.close_rows, j.close_kh, s)) return rc;
        at += rows_bytes(j.close_kh);
        B.expand[k] = element_of(j.expand_kw, j.expand_kh, j.expand_rows, at);
        if (int rc = stage_rows(at, j.expand_rows, j.expand_kh, s)) return rc;
        at += rows_bytes(j.expand_kh);
    }
    HIP_TRY(hipStreamSynchronize(s));                     // the caller's element rows are read; the earlier batch is done with the scratch
    return 0;
}
// both go from the held plane into the other one, which the jobs that took the step hold afterwards
int finish_morph(FinishBatch& B, hipStream_t s, const Element* el, int flags) {
    if (int rc = morph_step(B.mk, s, [&](int k) { return B.held(k); }, [&](int k) { return B.other(k); }, el, flags)) return rc;
    for (int k = 0; k < B.mk.n_jobs; ++k) B.cur[k] ^= el[k].kh != 0;
    return 0;
}
// the edge fuse of the jobs that have strips: the copy, then the fills
int finish_fuse(FinishBatch& B, hipStream_t s) {
    for (int phase = 0; phase < 2; ++phase) {
        B.mk.phase = phase;
        if (int rc = run_step(B.mk, launch_mask_fuse, s, [&](int k, MkJob& J) -> int64_t {
                if (!J.f) return 0;
                J.in = B.held(k); J.out = B.other(k);
                return mk_item_tiles(phase ? mk_fuse_items(J) : mk_plane_items(J));
            })) return rc;
    }
    for (int k = 0; k < B.mk.n_jobs; ++k) B.cur[k] ^= B.mk.job[k].f != 0;
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
    hipStream_t s;
    if (int rc = begin_call(c, slot, n_jobs, scratch_dev, scratch_bytes, need, counts_dev, &s)) return rc;
    for (int k0 = 0; k0 < n_jobs; k0 += GS360_MAX_VIEWS) {
        FinishBatch B;
        if (int rc = finish_batch(B, jobs + k0, std::min(GS360_MAX_VIEWS, n_jobs - k0), (uint8_t*)scratch_dev, counts_dev + k0, s)) return rc;
        if (int rc = run_step(B.mk, launch_mask_pack_bits, s, [&](int k, MkJob& J) { J.out = B.held(k); return row_tiles(J, kMkPackTile); })) return rc;
        if (int rc = finish_morph(B, s, B.close, 0)) return rc;                          // close: dilate ...
        if (int rc = finish_morph(B, s, B.close, kMkCompIn | kMkCompOut)) return rc;     // ... then erode
        if (int rc = finish_morph(B, s, B.expand, 0)) return rc;                         // expand
        if (int rc = finish_fuse(B, s)) return rc;
        for (int phase = 0; phase < 2; ++phase) {                                        // add layer and count, then the output
            B.mk.phase = phase;
            if (int rc = run_step(B.mk, launch_mask_finish, s, [&](int k, MkJob& J) {
                    J.out = B.held(k);
                    return row_tiles(J, phase ? mk_output_tile(J.kind) : kMkCountTile);
                })) return rc;
        }
    }
    return GS360_OK;
}

// ---- the shadow estimate (MSK-SHADOW v1): gs360_maskshadow.hip's kernels around the morph kernel above ---------------------------
namespace {

// a job's area of the scratch; it depends on H and W alone, so both calls and the caller find a job's planes in the same place
enum { kShP, kShC0, kShC1, kShC2, kShClean, kShSat, kShT0, kShT1, kShPlanes };
enum { kShElClose, kShElNear, kShElSclose, kShElOpen, kShElements };
constexpr size_t kShHead = 256;                           // the call's error word, in front of the first job's area
struct ShadowArea {
    size_t plane, gray, mid, area, weights, sdiv, rows[kShElements], total;
};
ShadowArea shadow_area(int H, int W) {
    ShadowArea a;
    size_t at = kShPlanes * plane_bytes(H, W);
    a.plane = plane_bytes(H, W);
    a.gray = at; at += round_up((size_t)H * ((size_t)(W + 31) / 32) * 32, 256);
    a.mid = at; at += round_up((size_t)H * W * 4, 256);
    a.area = at; at += round_up((size_t)H * W * 4, 256);
    a.weights = at; at += round_up((size_t)(kMsMaxR + 1) * 4, 256);
    a.sdiv = at; at += 1024;
    for (int e = 0; e < kShElements; ++e) { a.rows[e] = at; at += rows_bytes(GS360_MASK_MAX_ELEMENT); }
    a.total = at;
    return a;
}

int check_shadow_job(int k, const gs360_shadow_job& j, bool merge) {
    if (j.H < 1 || j.W < 1) return fail(GS360_ERR_ARG, "job %d: image of %d x %d", k, j.W, j.H);
    if (j.H > GS360_MASK_MAX_SIDE || j.W > GS360_MASK_MAX_SIDE)
        return fail(GS360_ERR_UNSUPPORTED, "job %d: image sides are 1..%d (got %d x %d)", k, GS360_MASK_MAX_SIDE, j.W, j.H);
    if ((int64_t)j.H * j.W > GS360_SHADOW_MAX_PIXELS)
        return fail(GS360_ERR_UNSUPPORTED, "job %d: %d x %d is above 2^30 pixels (labels are 32-bit, areas are doubled)", k, j.W, j.H);
    if (j.radius < 0) return fail(GS360_ERR_ARG, "job %d: filter radius %d", k, j.radius);
    if (j.radius > GS360_SHADOW_MAX_RADIUS) return fail(GS360_ERR_UNSUPPORTED, "job %d: filter radius %d above %d", k, j.radius, GS360_SHADOW_MAX_RADIUS);
    if ((j.src_stride && j.src_stride < (size_t)j.W) || (j.image_stride && j.image_stride < (size_t)j.W * 3) || (j.dst_stride && j.dst_stride < (size_t)j.W))
        return fail(GS360_ERR_ARG, "job %d: a stride below a row", k);
    if (!merge) {
        if (!j.image || !j.weights || !j.sdiv) return fail(GS360_ERR_ARG, "job %d: NULL image, weights or divisor table", k);
        if (j.thresh < 0 || j.thresh > 255) return fail(GS360_ERR_ARG, "job %d: thresh %d outside 0..255", k, j.thresh);
        return check_element(k, "close", j.close_kw, j.close_kh, j.close_rows);
    }
    if (!j.dst) return fail(GS360_ERR_ARG, "job %d: NULL output", k);
    if (j.near_kh < 1 || j.sclose_kh < 1 || j.open_kh < 1) return fail(GS360_ERR_ARG, "job %d: the merge needs its three elements", k);
    if (int rc = check_element(k, "near", j.near_kw, j.near_kh, j.near_rows)) return rc;
    if (int rc = check_element(k, "shadow close", j.sclose_kw, j.sclose_kh, j.sclose_rows)) return rc;
    return check_element(k, "open", j.open_kw, j.open_kh, j.open_rows);
}

int check_shadow_jobs(const gs360_shadow_job* jobs, int n_jobs, bool merge, size_t* need) {
    if (n_jobs < 0) return fail(GS360_ERR_ARG, "n_jobs < 0");
    if (n_jobs && !jobs) return fail(GS360_ERR_ARG, "NULL argument");
    *need = kShHead;
    for (int k = 0; k < n_jobs; ++k) {
        if (int rc = check_shadow_job(k, jobs[k], merge)) return rc;
        *need += shadow_area(jobs[k].H, jobs[k].W).total;
    }
    return 0;
}

// a job's four elements as the caller gives them, by kShEl... index; the candidates take the first, the merge the other three
struct ShadowElements {
    int kw[kShElements], kh[kShElements];
    const int32_t* rows[kShElements];
    explicit ShadowElements(const gs360_shadow_job& j)
        : kw{j.close_kw, j.near_kw, j.sclose_kw, j.open_kw}, kh{j.close_kh, j.near_kh, j.sclose_kh, j.open_kh},
          rows{j.close_rows, j.near_rows, j.sclose_rows, j.open_rows} {}
    static int first(bool merge) { return merge ? kShElNear : kShElClose; }
    static int end(bool merge) { return merge ? kShElements : kShElNear; }
};

// the jobs [k0, k0 + n) of a call as one launch of either family; base[k]: the job's area of the scratch
struct ShadowBatch {
    MkLaunch mk;
    MsLaunch ms;
    uint8_t* base[GS360_MAX_VIEWS];
    ShadowArea area[GS360_MAX_VIEWS];
    Element el[kShElements][GS360_MAX_VIEWS];             // those of the call
    uint32_t* plane(int k, int which) const { return (uint32_t*)(base[k] + (size_t)which * area[k].plane); }
};
// fills B from the jobs at *at of the scratch and moves *at behind them
void shadow_batch(ShadowBatch& B, const gs360_shadow_job* jobs, int n, bool merge, uint8_t** at, uint32_t* counts, uint32_t* err) {
    std::memset(&B.mk, 0, sizeof(B.mk));
    std::memset(&B.ms, 0, sizeof(B.ms));
    B.mk.n_jobs = B.ms.n_jobs = n;
    B.mk.counts = B.ms.counts = counts;
    B.ms.err = err;
    for (int k = 0; k < n; ++k) {
        const gs360_shadow_job& j = jobs[k];
        B.base[k] = *at;
        B.area[k] = shadow_area(j.H, j.W);
        *at += B.area[k].total;
        MkJob& K = B.mk.job[k];
        K.src = (const uint8_t*)j.src;
        K.src_stride = stride_or(j.src_stride, (size_t)j.W);
        K.H = j.H; K.W = j.W; K.pw = (j.W + 31) / 32; K.thresh = j.thresh;
        MsJob& S = B.ms.job[k];
        S.img = (const uint8_t*)j.image; S.dst = (uint8_t*)j.dst;
        S.img_stride = stride_or(j.image_stride, (size_t)j.W * 3);
        S.dst_stride = stride_or(j.dst_stride, (size_t)j.W);
        S.gray = B.base[k] + B.area[k].gray;
        S.mid = (float*)(B.base[k] + B.area[k].mid); S.lab = (int32_t*)S.mid;
        S.area = (uint32_t*)(B.base[k] + B.area[k].area);
        S.k = (const float*)(B.base[k] + B.area[k].weights); S.sdiv = (const int32_t*)(B.base[k] + B.area[k].sdiv);
        S.H = j.H; S.W = j.W; S.pw = K.pw; S.r = j.radius;
        S.t = j.t; S.delta_min = j.delta_min; S.sat_max = j.sat_max;
        S.th2 = (uint32_t)std::min<int64_t>(2 * (int64_t)std::max(1, j.min_area), UINT32_MAX);
        const ShadowElements el(j);
        for (int e = el.first(merge); e < el.end(merge); ++e) B.el[e][k] = element_of(el.kw[e], el.kh[e], el.rows[e], B.base[k] + B.area[k].rows[e]);
    }
}
// one dilate or erode of every job of the batch: plane `from` -> plane `to` by element e
int shadow_morph(ShadowBatch& B, hipStream_t s, int from, int to, int e, int flags) {
    return morph_step(B.mk, s, [&](int k) { return B.plane(k, from); }, [&](int k) { return B.plane(k, to); }, B.el[e], flags);
}
// one step of gs360_maskshadow.hip over the batch
template <class Tiles>
int shadow_step(ShadowBatch& B, hipStream_t s, MsStep step, Tiles tiles_of) {
    return run_step(B.ms, [step](const MsLaunch& L, hipStream_t st) { return launch_mask_shadow(step, L, st); }, s, tiles_of);
}
// labels of plane `which` (or of its complement) of every job: init, merge with connectivity `conn`, flatten
int shadow_label(ShadowBatch& B, hipStream_t s, int which, int conn, int flags) {
    B.ms.conn = conn;
    for (MsStep step : {kMsLabelInit, kMsLabelMerge, kMsLabelFlatten})
        if (int rc = shadow_step(B, s, step, [&](int k, MsJob& J) {
                J.a = B.plane(k, which); J.flags = flags;
                return mk_item_tiles(mk_plane_items(J));
            })) return rc;
    return 0;
}

// either call: the checks, the caller's tables and elements staged in every job's area and read, then `steps(B, s)` per batch
template <class Steps>
int shadow_call(gs360_ctx* c, const gs360_shadow_job* jobs, int n_jobs, bool merge, void* scratch_dev, size_t scratch_bytes,
                uint32_t* counts_dev, int slot, hipStream_t* s, Steps steps) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    size_t need = 0;
    if (int rc = check_shadow_jobs(jobs, n_jobs, merge, &need)) return rc;
    if (n_jobs == 0) return 0;
    if (int rc = begin_call(c, slot, n_jobs, scratch_dev, scratch_bytes, need, counts_dev, s)) return rc;
    if (merge) HIP_TRY(hipMemsetAsync(scratch_dev, 0, kShHead, *s));
    uint8_t* at = (uint8_t*)scratch_dev + kShHead;
    for (int k = 0; k < n_jobs; ++k) {
        const gs360_shadow_job& j = jobs[k];
        const ShadowArea a = shadow_area(j.H, j.W);
        const ShadowElements el(j);
        for (int e = el.first(merge); e < el.end(merge); ++e)
            if (int rc = stage_rows(at + a.rows[e], el.rows[e], el.kh[e], *s)) return rc;
        if (!merge) {
            HIP_TRY(hipMemcpyAsync(at + a.weights, j.weights, (size_t)(j.radius + 1) * 4, hipMemcpyHostToDevice, *s));
            HIP_TRY(hipMemcpyAsync(at + a.sdiv, j.sdiv, 1024, hipMemcpyHostToDevice, *s));
        }
        at += a.total;
    }
    HIP_TRY(hipStreamSynchronize(*s));                    // the caller's tables and element rows are read
    at = (uint8_t*)scratch_dev + kShHead;
    for (int k0 = 0; k0 < n_jobs; k0 += GS360_MAX_VIEWS) {
        ShadowBatch B;
        shadow_batch(B, jobs + k0, std::min(GS360_MAX_VIEWS, n_jobs - k0), merge, &at, counts_dev + k0, (uint32_t*)scratch_dev);
        if (int rc = steps(B, *s)) return rc;
    }
    return 0;
}

}  // namespace

int gs360_mask_shadow_scratch(const gs360_shadow_job* jobs, int n_jobs, size_t* bytes) {
    if (!bytes) return fail(GS360_ERR_ARG, "NULL argument");
    size_t need = 0;
    if (int rc = check_shadow_jobs(jobs, n_jobs, false, &need)) return rc;
    *bytes = need;
    return GS360_OK;
}

int gs360_mask_shadow_candidates_u8(gs360_ctx* c, const gs360_shadow_job* jobs, int n_jobs, void* scratch_dev, size_t scratch_bytes,
                                    uint32_t* counts_dev, int slot) {
    hipStream_t stream;
    return shadow_call(c, jobs, n_jobs, false, scratch_dev, scratch_bytes, counts_dev, slot, &stream, [](ShadowBatch& B, hipStream_t s) {
        const Element* close = B.el[kShElClose];
        // P: MSK-SPEC steps 0-1 (pack, close); a job without a close packs straight into P
        if (int rc = run_step(B.mk, launch_mask_pack_bits, s, [&](int k, MkJob& J) { J.out = B.plane(k, close[k].kh ? kShT0 : kShP); return row_tiles(J, kMkPackTile); })) return rc;
        if (int rc = shadow_morph(B, s, kShT0, kShT1, kShElClose, 0)) return rc;
        if (int rc = shadow_morph(B, s, kShT1, kShP, kShElClose, kMkCompIn | kMkCompOut)) return rc;
        B.mk.phase = 0;                                   // count(P): the finishing chain's counting pass without an add layer
        if (int rc = run_step(B.mk, launch_mask_finish, s, [&](int k, MkJob& J) { J.out = B.plane(k, kShP); return row_tiles(J, kMkCountTile); })) return rc;
        if (int rc = shadow_step(B, s, kMsPixel, [&](int k, MsJob& J) { J.out = B.plane(k, kShSat); return row_tiles(J, kMsPixelTile); })) return rc;
        if (int rc = shadow_step(B, s, kMsBlurRows, [&](int, MsJob& J) { return row_tiles(J, kMsRowsTile); })) return rc;
        return shadow_step(B, s, kMsBlurCols, [&](int k, MsJob& J) {
            J.a = B.plane(k, kShSat); J.out = B.plane(k, kShC0);
            return row_tiles(J, kMsColsTile);
        });
    });
}

int gs360_mask_shadow_merge_u8(gs360_ctx* c, const gs360_shadow_job* jobs, int n_jobs, void* scratch_dev, size_t scratch_bytes,
                               uint32_t* counts_dev, int slot) {
    hipStream_t s;
    if (int rc = shadow_call(c, jobs, n_jobs, true, scratch_dev, scratch_bytes, counts_dev, slot, &s, [](ShadowBatch& B, hipStream_t s) {
            auto clear_area = [&]() {
                for (int k = 0; k < B.ms.n_jobs; ++k) HIP_TRY(hipMemsetAsync(B.ms.job[k].area, 0, (size_t)B.ms.job[k].H * B.ms.job[k].W * 4, s));
                return 0;
            };
            const int both = kMkCompIn | kMkCompOut;
            if (int rc = shadow_morph(B, s, kShP, kShT0, kShElNear, 0)) return rc;                             // step 4: the near region
            if (int rc = shadow_step(B, s, kMsLogic, [&](int k, MsJob& J) {
                    J.a = B.plane(k, kShC0); J.b = B.plane(k, kShT0); J.c = B.plane(k, kShP); J.out = B.plane(k, kShC1);
                    return mk_item_tiles(mk_plane_items(J));
                })) return rc;
            if (int rc = shadow_morph(B, s, kShC1, kShT0, kShElSclose, 0)) return rc;                          // step 5: close ...
            if (int rc = shadow_morph(B, s, kShT0, kShT1, kShElSclose, both)) return rc;
            if (int rc = shadow_morph(B, s, kShT1, kShT0, kShElOpen, both)) return rc;                         // ... and open
            if (int rc = shadow_morph(B, s, kShT0, kShC2, kShElOpen, 0)) return rc;
            if (int rc = clear_area()) return rc;                                                              // step 6: O, G = ~O in T1
            if (int rc = shadow_label(B, s, kShC2, 4, kMsComplement)) return rc;
            if (int rc = shadow_step(B, s, kMsBorder, [&](int, MsJob& J) { return mk_item_tiles(ms_border_items(J)); })) return rc;
            if (int rc = shadow_step(B, s, kMsFill, [&](int k, MsJob& J) { J.out = B.plane(k, kShT1); return row_tiles(J, kMsFillTile); })) return rc;
            if (int rc = clear_area()) return rc;
            if (int rc = shadow_label(B, s, kShT1, 8, 0)) return rc;
            if (int rc = shadow_step(B, s, kMsArea, [&](int k, MsJob& J) { J.a = B.plane(k, kShT1); return mk_item_tiles(ms_area_items(J)); })) return rc;
            return shadow_step(B, s, kMsSelect, [&](int k, MsJob& J) {                                         // steps 6-7: clean, M and its count
                J.a = B.plane(k, kShT1); J.b = B.plane(k, kShP); J.out = B.plane(k, kShClean);
                return row_tiles(J, kMsSelectTile);
            });
        })) return rc;
    if (n_jobs == 0) return GS360_OK;
    uint32_t err = 0;                                     // a label walk past its bound: the result is not to be used
    HIP_TRY(hipMemcpyAsync(&err, scratch_dev, sizeof(err), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (err) return fail(GS360_ERR_INTERNAL, "a label walk ran past its bound");
    return GS360_OK;
}

// ---- inpainting the masked region (MSK-INPAINT v1): gs360_maskinpaint.hip's kernels ----------------------------------------------
namespace {

constexpr size_t kMiHeadBytes = (sizeof(MiHead) + 255) / 256 * 256;
constexpr size_t kMiTableBytes = (size_t)kMiMaxOffsets * 16 / 256 * 256 + 256;   // per job: (dy, dx) pairs, |r|, 1 / |r|^2
// a job's area of the scratch behind the head: its offset table, then vert, lev and dist
struct InpaintArea { size_t vert, lev, dist, total; };
InpaintArea inpaint_area(int H, int W) {
    InpaintArea a;
    const size_t px = (size_t)H * W;
    a.vert = kMiTableBytes;
    a.lev = a.vert + round_up(px * 2, 256);
    a.dist = a.lev + round_up(px * 2, 256);
    a.total = a.dist + round_up(px * 4, 256);
    return a;
}

int check_inpaint_job(int k, const gs360_inpaint_job& j) {
    if (j.H < 1 || j.W < 1) return fail(GS360_ERR_ARG, "job %d: image of %d x %d", k, j.W, j.H);
    if (j.H > GS360_MASK_MAX_SIDE || j.W > GS360_MASK_MAX_SIDE)
        return fail(GS360_ERR_UNSUPPORTED, "job %d: image sides are 1..%d (got %d x %d)", k, GS360_MASK_MAX_SIDE, j.W, j.H);
    if (!j.image || !j.fill) return fail(GS360_ERR_ARG, "job %d: NULL image or fill mask", k);
    if ((j.image_stride && j.image_stride < (size_t)j.W * 3) || (j.fill_stride && j.fill_stride < (size_t)j.W))
        return fail(GS360_ERR_ARG, "job %d: a stride below a row", k);
    if (j.radius < 1) return fail(GS360_ERR_ARG, "job %d: inpaint radius %d", k, j.radius);
    if (j.radius < 3 || j.radius > GS360_INPAINT_MAX_RADIUS)
        return fail(GS360_ERR_UNSUPPORTED, "job %d: inpaint radius %d outside 3..%d", k, j.radius, GS360_INPAINT_MAX_RADIUS);
    return 0;
}

// the jobs from k0 on that make one batch: at most GS360_MAX_VIEWS, their pixels numbered below 2^32 (a job has 2^30 at most)
int inpaint_batch_len(const gs360_inpaint_job* jobs, int k0, int n_jobs, uint64_t* pixels) {
    int n = 0;
    *pixels = 0;
    while (k0 + n < n_jobs && n < GS360_MAX_VIEWS && *pixels + (uint64_t)jobs[k0 + n].H * jobs[k0 + n].W <= UINT32_MAX) {
        *pixels += (uint64_t)jobs[k0 + n].H * jobs[k0 + n].W;
        ++n;
    }
    return n;
}

int check_inpaint_jobs(const gs360_inpaint_job* jobs, int n_jobs, size_t* need) {
    if (n_jobs < 0) return fail(GS360_ERR_ARG, "n_jobs < 0");
    if (n_jobs && !jobs) return fail(GS360_ERR_ARG, "NULL argument");
    *need = 0;
    for (int k = 0; k < n_jobs; ++k)
        if (int rc = check_inpaint_job(k, jobs[k])) return rc;
    uint64_t pixels;
    for (int k0 = 0, n; k0 < n_jobs; k0 += n) {           // a batch's scratch: the head, the jobs' areas, the list
        n = inpaint_batch_len(jobs, k0, n_jobs, &pixels);
        size_t b = kMiHeadBytes + round_up((size_t)pixels * 4, 256);
        for (int k = k0; k < k0 + n; ++k) b += inpaint_area(jobs[k].H, jobs[k].W).total;
        *need = std::max(*need, b);
    }
    return 0;
}

// the offsets (dy, dx) with 0 < dy^2 + dx^2 <= radius^2 in row-major order, |r| and 1 / |r|^2 in double rounded to float32, laid
// out as a job's table -> their number
int inpaint_table(int radius, uint8_t* table) {
    int32_t* off = (int32_t*)table;
    float *rlen = (float*)(table + (size_t)kMiMaxOffsets * 8), *inv2 = rlen + kMiMaxOffsets;
    int n = 0;
    for (int dy = -radius; dy <= radius; ++dy)
        for (int dx = -radius; dx <= radius; ++dx) {
            const int d = dy * dy + dx * dx;
            if (d == 0 || d > radius * radius) continue;
            off[2 * n] = dy; off[2 * n + 1] = dx;
            rlen[n] = (float)std::sqrt((double)d); inv2[n] = (float)(1.0 / (double)d);
            ++n;
        }
    return n;
}

template <class Tiles>
int inpaint_step(MiLaunch& L, hipStream_t s, MiStep step, Tiles tiles_of) {
    return run_step(L, [step](const MiLaunch& l, hipStream_t st) { return launch_mask_inpaint(step, l, st); }, s, tiles_of);
}

}  // namespace

int gs360_mask_inpaint_scratch(const gs360_inpaint_job* jobs, int n_jobs, size_t* bytes) {
    if (!bytes) return fail(GS360_ERR_ARG, "NULL argument");
    size_t need = 0;
    if (int rc = check_inpaint_jobs(jobs, n_jobs, &need)) return rc;
    *bytes = need;
    return GS360_OK;
}

int gs360_mask_inpaint_u8(gs360_ctx* c, const gs360_inpaint_job* jobs, int n_jobs, void* scratch_dev, size_t scratch_bytes,
                          uint32_t* levels_dev, int slot) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    size_t need = 0;
    if (int rc = check_inpaint_jobs(jobs, n_jobs, &need)) return rc;
    if (n_jobs == 0) return GS360_OK;
    hipStream_t s;
    if (int rc = begin_call(c, slot, n_jobs, scratch_dev, scratch_bytes, need, levels_dev, &s)) return rc;
    MiHead* head = (MiHead*)scratch_dev;
    HIP_TRY(hipMemsetAsync(head, 0, offsetof(MiHead, filled), s));                     // the error word: once per call
    std::vector<uint8_t> tables((size_t)GS360_MAX_VIEWS * kMiTableBytes);
    std::vector<uint32_t> seen(offsetof(MiHead, offs) / 4);                              // the head up to the histogram's end
    uint64_t pixels;
    for (int k0 = 0, n; k0 < n_jobs; k0 += n) {
        n = inpaint_batch_len(jobs, k0, n_jobs, &pixels);
        MiLaunch L;
        std::memset(&L, 0, sizeof(L));
        L.n_jobs = n; L.head = head; L.levels = levels_dev + k0; L.list_cap = (uint32_t)pixels;
        HIP_TRY(hipMemsetAsync(head->filled, 0, sizeof(MiHead) - offsetof(MiHead, filled), s));
        uint8_t* at = (uint8_t*)scratch_dev + kMiHeadBytes;
        uint32_t base = 0;
        for (int k = 0; k < n; ++k) {
            const gs360_inpaint_job& j = jobs[k0 + k];
            const InpaintArea a = inpaint_area(j.H, j.W);
            MiJob& J = L.job[k];
            J.img = (uint8_t*)j.image; J.fill = (const uint8_t*)j.fill;
            J.img_stride = stride_or(j.image_stride, (size_t)j.W * 3);
            J.fill_stride = stride_or(j.fill_stride, (size_t)j.W);
            J.H = j.H; J.W = j.W; J.px_base = base;
            base += (uint32_t)j.H * (uint32_t)j.W;
            J.n_off = inpaint_table(j.radius, tables.data() + (size_t)k * kMiTableBytes);
            J.off = (const int32_t*)at; J.rlen = (const float*)(at + (size_t)kMiMaxOffsets * 8); J.inv2 = J.rlen + kMiMaxOffsets;
            J.vert = (uint16_t*)(at + a.vert); J.lev = (uint16_t*)(at + a.lev); J.dist = (float*)(at + a.dist);
            HIP_TRY(hipMemcpyAsync(at, tables.data() + (size_t)k * kMiTableBytes, kMiTableBytes, hipMemcpyHostToDevice, s));
            at += a.total;
        }
        L.list = (uint32_t*)at;
        if (int rc = inpaint_step(L, s, kMiCols, [&](int, MiJob& J) { return mk_item_tiles(mi_cols_items(J)); })) return rc;
        if (int rc = inpaint_step(L, s, kMiRows, [&](int, MiJob& J) { return row_tiles(J, kMiRowTile); })) return rc;
        L.total_tiles = 1;
        HIP_TRY(launch_mask_inpaint(kMiScan, L, s));
        if (int rc = inpaint_step(L, s, kMiScatter, [&](int, MiJob& J) { return row_tiles(J, kMiRowTile); })) return rc;
        // the one read of the batch: the error word so far, the pixels per level (the tables above are read by now as well)
        HIP_TRY(hipMemcpyAsync(seen.data(), head, seen.size() * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (seen[0]) return fail(GS360_ERR_INTERNAL, "an inpaint lane left its bound");
        const uint32_t* hist = seen.data() + offsetof(MiHead, hist) / 4;
        if (hist[kMiFar]) return fail(GS360_ERR_UNSUPPORTED, "a masked region is deeper than %d levels", kMiMaxLevel);
        for (int level = 1; level <= kMiMaxLevel; ++level) {
            if (!hist[level]) continue;                  // (the levels of a batch have no gaps; an empty one has nothing to launch)
            L.level = level; L.items = hist[level];
            L.total_tiles = (int32_t)mk_item_tiles(hist[level]);
            HIP_TRY(launch_mask_inpaint(kMiFill, L, s));
        }
    }
    uint32_t err = 0;                                     // a fill lane that left its bound: the result is not to be used
    HIP_TRY(hipMemcpyAsync(&err, head, sizeof(err), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (err) return fail(GS360_ERR_INTERNAL, "an inpaint lane left its bound");
    return GS360_OK;
}
