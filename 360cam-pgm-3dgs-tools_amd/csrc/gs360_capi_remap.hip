// gs360_capi_remap.hip -- C-ABI glue of the cv2-style remaps (include/gs360.h): OpenCV's interpolation weight tables, map plans,
// the table remap of 8- and 16-bit images (float maps or map plans), the fused fisheye -> views path and the remap host conveniences.
#include "gs360_capi_internal.h"

using namespace gs360;

struct gs360_map_plan {         // float maps packed once (gs360_table.hip, map plans)
    int device = 0;
    int h = 0, w = 0;
    int nearest = 0;
    int has_valid = 0;
    uint32_t* d_packed = nullptr;
    uint8_t* d_hi = nullptr;
    // stage plans of this map (gs360_tablestage.hip), one per (source size, tile rows, valid bit applied): built at the first call that asks
    mutable std::mutex ts_mutex;
    mutable std::vector<gs360::TsPlan*> ts_plans;
};

// OpenCV imgproc initInterTab2D(fixed point), restated: per-phase 1-D coefficients in float32, outer product scaled
// by 2^15 and rounded to short, then the entries are patched so each ks x ks kernel sums to 2^15 (the patch goes to
// the largest / smallest entry of rows/cols ks/2 .. ks/2+1, the block OpenCV inspects).
namespace {
void build_tab2d(const float* c1, int ks, int16_t* out) {
    const int h = ks / 2;
    for (int fy = 0; fy < 32; ++fy)
        for (int fx = 0; fx < 32; ++fx) {
            int16_t* k = out + (fy * 32 + fx) * ks * ks;
            int sum = 0;
            for (int a = 0; a < ks; ++a)
                for (int b = 0; b < ks; ++b) {
                    long r = std::lrintf(c1[fy * ks + a] * c1[fx * ks + b] * 32768.0f);
                    r = r < -32768 ? -32768 : (r > 32767 ? 32767 : r);
                    k[a * ks + b] = (int16_t)r;
                    sum += (int)r;
                }
            if (sum != 32768) {
                int hi = h * ks + h, lo = hi;
                for (int a = h; a < h + 2; ++a)
                    for (int b = h; b < h + 2; ++b) {
                        const int idx = a * ks + b;
                        if (k[idx] < k[lo]) lo = idx;
                        else if (k[idx] > k[hi]) hi = idx;
                    }
                const int diff = sum - 32768;
                if (diff < 0) k[hi] = (int16_t)(k[hi] - diff);
                else k[lo] = (int16_t)(k[lo] - diff);
            }
        }
}

void cubic_coef1d(float* c1) {   // Keys kernel, A = -0.75: 32 phases x 4 taps
    const float A = -0.75f;
    for (int i = 0; i < 32; ++i) {
        const float x = (float)i * (1.0f / 32.0f);
        float* c = c1 + i * 4;
        c[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
        c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
        c[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
        c[3] = 1.f - c[0] - c[1] - c[2];
    }
}

void lanczos4_coef1d(float* c1) {   // OpenCV interpolateLanczos4: taps -3..+4, one sin/cos pair per phase; 32 phases x 8 taps
    static const double r = 0.70710678118654752440084436210485;
    static const double rot[8][2] = {{1, 0}, {-r, -r}, {0, 1}, {r, -r}, {-1, 0}, {r, r}, {0, -1}, {-r, r}};
    for (int i = 0; i < 32; ++i) {
        const float x = (float)i * (1.0f / 32.0f);
        float* c = c1 + i * 8;
        if (x < 1.1920928955078125e-07f) {
            for (int t = 0; t < 8; ++t) c[t] = (t == 3) ? 1.f : 0.f;
            continue;
        }
        const double a0 = -(x + 3) * kPi * 0.25, s0 = std::sin(a0), c0 = std::cos(a0);
        float sum = 0.f;
        for (int t = 0; t < 8; ++t) {
            const double a = -(x + 3 - t) * kPi * 0.25;
            c[t] = (float)((rot[t][0] * s0 + rot[t][1] * c0) / (a * a));
            sum += c[t];
        }
        sum = 1.f / sum;
        for (int t = 0; t < 8; ++t) c[t] *= sum;
    }
}

constexpr int kTsBoxBudget = 26 * 1024 - 64;     // largest tile box of the LDS-staged table kernel: two of them per workgroup, three workgroups per CU
// its box loader splits chunk c into (c * magic) >> 21 rows, magic = ceil(2^21 / wch) (table_stage_plan_kernel): exact while chunks * wch <
// 2^21, no 32-bit overflow while rows < 2^11 -- for boxes as wide as a map plan's widest source (wch <= 766) and up to the budget's chunks
constexpr int kTsBoxChunks = kTsBoxBudget / 16, kTsMaxWch = ((((3 * (kMapPlanMaxDim - 1)) & ~3) + 12) + 15) >> 4;
static_assert(kTsBoxChunks * kTsMaxWch < (1 << 21) && kTsBoxChunks < (1 << 11), "the box loader's row split needs a wider magic");

uint8_t sat_u8(double v) {  // cv::saturate_cast<uchar>(double)
    long r = std::lrint(v);
    return (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
}

int check_map_plan(gs360_ctx* c, const gs360_remap_job& J, const gs360_map_plan* plan, int interp) {
    if (plan->device != c->device) return fail(GS360_ERR_ARG, "map plan belongs to device %d, ctx is device %d", plan->device, c->device);
    if (plan->h != J.h || plan->w != J.w) return fail(GS360_ERR_ARG, "map plan is %dx%d, the job asks for %dx%d", plan->w, plan->h, J.w, J.h);
    if (plan->nearest != (interp == GS360_INTERP_NEAREST ? 1 : 0))
        return fail(GS360_ERR_ARG, "map plan was packed for %s sampling", plan->nearest ? "nearest" : "interpolated");
    if (J.W > kMapPlanMaxDim || J.H > kMapPlanMaxDim)
        return fail(GS360_ERR_UNSUPPORTED, "map plans address sources up to %d x %d (got %dx%d): use the float maps", kMapPlanMaxDim,
                    kMapPlanMaxDim, J.W, J.H);
    if (J.valid && !plan->has_valid) return fail(GS360_ERR_ARG, "the job asks for a valid fill, the plan was made without a valid map");
    return 0;
}

// One job of a table call checked and turned into its launch block; 1: an empty job (nothing to launch).  16-bit jobs (esize 2) need
// even strides and keep the zeroed block plus the common fields: the 16-bit launcher takes their weights and border values itself.
int fill_table_job(gs360_ctx* c, const gs360_remap_job& J, const gs360_map_plan* plan, int C, int interp, const double* border_value,
                   int esize, TableLaunch* L) {
    if (!J.src || !J.dst || (!plan && (!J.map_x || !J.map_y))) return fail(GS360_ERR_ARG, "NULL argument");
    if (plan)
        if (int rc = check_map_plan(c, J, plan, interp)) return rc;
    if (J.H < 1 || J.W < 1 || J.H >= 32767 || J.W >= 32767) return fail(GS360_ERR_ARG, "source size %dx%d outside cv2.remap limits", J.W, J.H);
    if (J.h < 0 || J.w < 0 || J.h >= 32767 || J.w >= 32767) return fail(GS360_ERR_ARG, "bad map size %dx%d", J.w, J.h);
    if (J.h == 0 || J.w == 0) return 1;
    size_t src_stride = J.src_stride ? J.src_stride : (size_t)J.W * C * esize;
    size_t dst_stride = J.dst_stride ? J.dst_stride : (size_t)J.w * C * esize;
    if (src_stride < (size_t)J.W * C * esize || dst_stride < (size_t)J.w * C * esize) return fail(GS360_ERR_ARG, "stride smaller than a row");
    if (esize == 2 && ((src_stride | dst_stride) & 1)) return fail(GS360_ERR_ARG, "16-bit images need even strides");
    std::memset(L, 0, sizeof(*L));
    L->src = (const uint8_t*)J.src; L->map_x = J.map_x; L->map_y = J.map_y; L->valid = J.valid; L->dst = (uint8_t*)J.dst;
    if (plan) {                    // job.valid != NULL asks for the plan's valid bit (the pointer itself is not read)
        L->packed = plan->d_packed; L->packed_hi = plan->d_hi; L->use_valid = J.valid ? 1 : 0;
        L->map_x = L->map_y = nullptr; L->valid = nullptr;
    }
    L->H = J.H; L->W = J.W; L->h = J.h; L->w = J.w;
    L->src_stride = (int64_t)src_stride; L->dst_stride = (int64_t)dst_stride;
    L->interp = interp;
    const int fill_max = esize == 2 ? 65535 : 255;
    L->fill = J.fill_value < 0 ? 0 : (J.fill_value > fill_max ? fill_max : J.fill_value);
    if (esize == 2) return 0;
    for (int k = 0; k < 4; ++k) L->cval[k] = sat_u8(border_value ? border_value[k] : 0.0);
    L->cubic_tab = interp == GS360_INTERP_LANCZOS4 ? c->d_lanczos : c->d_cubic;
    if (interp == GS360_INTERP_LANCZOS4 && c->lz_rebuild && !opt(c, kOptLanczosTable)) {   // (option "lanczos_table": probes / A-B runs)
        L->lz_c1 = c->d_coef1d + 192;
        L->lz_cen = c->d_lz_cen;
    }
    L->pipelined = (J.W >= 8 && src_stride < ((size_t)1 << 24) && (uint64_t)src_stride * (uint64_t)J.H < ((uint64_t)1 << 32)) ? 1 : 0;
    // a tight output whose rows are not whole dwords (the default 1750-pixel views), float maps: spans of the flat output, dword stores
    // (cfg4 70.4-72.8 -> 54.9-57.4 us per pair; with a map plan the byte stores of the row form are as fast: 52.7 vs 54.8, so plans keep it)
    const bool rows_only = opt(c, kOptTableRows) != 0;      // (option "table_rows": A/B)
    L->flat = (!plan && dst_stride == (size_t)J.w * C && (dst_stride & 3) != 0 && (reinterpret_cast<uintptr_t>(J.dst) & 3) == 0 &&
               !rows_only) ? 1 : 0;
    return 0;
}

// LDS-staged table kernel (gs360_tablestage.hip): bilinear RGB through a map plan, dword-aligned source rows, an output whose quads
// start on dword boundaries (tight, or rows of whole dwords), and offsets within the kernel's 31- and 32-bit forms.
bool table_stage_eligible(const TableLaunch& L, const gs360_map_plan* plan, int C, int interp) {
    const bool quads_ok = ((uintptr_t)L.dst & 3) == 0 && (L.dst_stride == (int64_t)3 * L.w ? ((int64_t)L.h * L.w) % 4 == 0 : (L.w % 4 == 0 && L.dst_stride % 4 == 0));
    return plan && C == 3 && interp == GS360_INTERP_LINEAR && L.pipelined && quads_ok && ((uintptr_t)L.src & 3) == 0 &&
           L.src_stride % 4 == 0 && (int64_t)L.H * L.src_stride < ((int64_t)1 << 31) && (int64_t)L.h * L.dst_stride < ((int64_t)1 << 32) &&
           (int64_t)L.h * L.w < ((int64_t)1 << 30);
}

// The map plan's stage plan for this job's source size and tile rows R: looked up, or built at the first call that asks for it (one
// launch + one synchronisation of the slot's stream, under the map plan's lock).
int stage_plan_for(const gs360_map_plan* plan, const TableLaunch& L, int R, gs360_ctx* c, int slot, TsPlan** out) {
    std::lock_guard<std::mutex> lock(plan->ts_mutex);
    for (TsPlan* q : plan->ts_plans)
        if (q->W == L.W && q->H == L.H && q->R == R && q->use_valid == L.use_valid) { *out = q; return 0; }
    hipError_t he = hipSuccess;
    TsPlan* tp = ts_build_plan(plan->d_packed, plan->d_hi, L.h, L.w, L.W, L.H, R, L.use_valid, kTsBoxBudget, c->stream[slot], &he);
    if (!tp) return fail(he == hipSuccess || he == hipErrorOutOfMemory ? GS360_ERR_NOMEM : GS360_ERR_HIP, "stage plan setup failed: %s", hipGetErrorString(he));
    plan->ts_plans.push_back(tp);
    *out = tp;
    return 0;
}

gs360_remap_job one_job(const void* src, int H, int W, size_t src_stride, const float* map_x, const float* map_y, const uint8_t* valid,
                        int h, int w, int fill_value, void* dst, size_t dst_stride) {
    gs360_remap_job J;
    J.src = src; J.H = H; J.W = W; J.src_stride = src_stride; J.map_x = map_x; J.map_y = map_y; J.valid = valid;
    J.h = h; J.w = w; J.fill_value = fill_value; J.dst = dst; J.dst_stride = dst_stride;
    return J;
}

// Table remap of 8-bit (esize 1) or 16-bit (esize 2) images in launches of up to GS360_MAX_VIEWS jobs; `plans` NULL: float maps.
int remap_batches(gs360_ctx* c, const gs360_remap_job* jobs, const gs360_map_plan* const* plans, int n_jobs, int C, int interp,
                  const double* border_value, int slot, int esize) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    if (n_jobs < 0 || (n_jobs > 0 && !jobs)) return fail(GS360_ERR_ARG, "bad job list");
    if (int rc = check_channels(C)) return rc;
    if (int rc = check_table_interp(interp)) return rc;
    uint16_t cval16[4];                // border values of the 16-bit launcher: cv::saturate_cast<ushort>(double)
    for (int k = 0; k < 4; ++k) {
        long r = std::lrint(border_value ? border_value[k] : 0.0);
        cval16[k] = (uint16_t)(r < 0 ? 0 : (r > 65535 ? 65535 : r));
    }
    HIP_TRY(hipSetDevice(c->device));
    int staged_jobs = 0, slow_tiles = 0;        // the whole call's, over all its launches (read-only options last_table_*)
    for (int j0 = 0; j0 < n_jobs; j0 += GS360_MAX_VIEWS) {
        TableBatch B;
        B.n_jobs = 0;
        B.persist_blocks = esize == 1 ? c->prop.multiProcessorCount * 8 : 0;     // 8-bit: two rounds of the four workgroups a CU holds (bicubic RGB)
        if (const int v = opt(c, kOptTablePersist); esize == 1 && v >= 0) B.persist_blocks = v;   // option "table_persist" (probes): 0 = one tile per workgroup
        // 8-bit jobs that can take the LDS-staged kernel.  Their stage plans are built at the first call.  Option "table_stage": 0 never,
        // 1 every job that can, -1 (default) those whose plan has boxes for at least 7/8 of its tiles (a map that scatters its taps --
        // random test maps -- would be redone pixel by pixel from memory).
        TsLaunch S;
        std::memset(&S, 0, sizeof(S));
        const int opt_stage = opt(c, kOptTableStage);
        S.R = opt(c, kOptTableStageRows);
        S.wg_per_cu = opt(c, kOptTableStageWgs);
        for (int j = j0; j < n_jobs && j < j0 + GS360_MAX_VIEWS; ++j) {
            if (esize == 1 && (jobs[j].h == 0 || jobs[j].w == 0)) continue;     // (8-bit: an empty job is skipped unchecked; 16-bit: checked first)
            const gs360_map_plan* plan = plans ? plans[j] : nullptr;
            TableLaunch& L = B.job[B.n_jobs];
            const int rc = fill_table_job(c, jobs[j], plan, C, interp, border_value, esize, &L);
            if (rc < 0) return rc;
            if (rc > 0) continue;
            if (esize == 1 && opt_stage != 0 && table_stage_eligible(L, plan, C, interp)) {
                TsPlan* tp = nullptr;
                if (int rc = stage_plan_for(plan, L, S.R, c, slot, &tp)) return rc;
                if (opt_stage == 1 || tp->slow_tiles * 8 <= tp->n_tiles) {
                    TsJobDesc& D = S.job[S.n_jobs++];
                    D.src = L.src; D.dst = L.dst; D.packed = L.packed; D.packed_hi = L.packed_hi; D.plan = tp;
                    D.src_stride = L.src_stride; D.dst_stride = L.dst_stride; D.fill = L.fill;
                    for (int k = 0; k < 4; ++k) S.cval[k] = L.cval[k];
                    slow_tiles += tp->slow_tiles;
                    continue;                            // (B.job[B.n_jobs] is overwritten by the next job)
                }
            }
            ++B.n_jobs;
        }
        if (esize == 2 && B.n_jobs) HIP_TRY(launch_table_u16_batch(B, C, c->d_coef1d, cval16, c->stream[slot]));
        if (esize == 2) continue;
        if (S.n_jobs) HIP_TRY(ts_launch(S, c->prop.multiProcessorCount, 160 * 1024, c->stream[slot]));
        if (B.n_jobs) HIP_TRY(launch_table_batch(B, C, c->stream[slot]));
        staged_jobs += S.n_jobs;
    }
    if (esize == 1) {
        c->last_table_kernel.store(staged_jobs, std::memory_order_relaxed);
        c->last_table_slow.store(slow_tiles, std::memory_order_relaxed);
    }
    return GS360_OK;
}

void make_fe_view(const gs360_calib& cal, const gs360_view& v, double lens_fov_deg, FeView* o) {
    double hf = clampd(v.hfov_deg, 1e-3, 179.9) * kPi / 180.0;
    double vf = clampd(v.vfov_deg, 1e-3, 179.9) * kPi / 180.0;
    o->sxu = (float)(std::tan(hf * 0.5) / (double)v.width);
    o->syv = (float)(std::tan(vf * 0.5) / (double)v.height);
    double pitch = v.pitch_deg * kPi / 180.0, yaw = v.yaw_deg * kPi / 180.0;
    o->sp = (float)std::sin(pitch); o->cp = (float)std::cos(pitch);
    o->sy = (float)std::sin(yaw); o->cy = (float)std::cos(yaw);
    o->k1 = (float)cal.k1; o->k2 = (float)cal.k2; o->k3 = (float)cal.k3; o->k4 = (float)cal.k4;
    o->p1 = (float)cal.p1; o->p2 = (float)cal.p2;
    o->tp1 = (float)(2.0 * cal.p1); o->tp2 = (float)(2.0 * cal.p2);
    o->b1 = (float)cal.b1; o->b2 = (float)cal.b2; o->f = (float)cal.f;
    o->cx0 = (float)((cal.width * 0.5) + cal.cx);   // DF:1812-1813
    o->cy0 = (float)((cal.height * 0.5) + cal.cy);
    o->wmax = (float)(cal.width - 1); o->hmax = (float)(cal.height - 1);
    o->cos_tmax = (float)std::cos(clampd(lens_fov_deg, 1.0, 360.0) * 0.5 * kPi / 180.0);  // DF:1800
    o->tang = (cal.p1 != 0.0 || cal.p2 != 0.0) ? 1 : 0;
    o->W = cal.width; o->H = cal.height;
    o->out_w = v.width; o->out_h = v.height;
    o->tiles_x = (v.width + kTileW - 1) / kTileW;
    o->tiles_y = (v.height + kTileH - 1) / kTileH;
}

int remap_table_host_impl(gs360_ctx* c, const void* src, int H, int W, int C, size_t src_stride, const float* map_x,
                          const float* map_y, const uint8_t* valid, int h, int w, int interp,
                          const double* border_value, int fill_value, void* dst, size_t dst_stride, int slot, int esize) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    if (!src || !map_x || !map_y || !dst) return fail(GS360_ERR_ARG, "NULL argument");
    if (int rc = check_channels(C)) return rc;
    if (H < 1 || W < 1 || h < 0 || w < 0) return fail(GS360_ERR_ARG, "bad size");
    if (h == 0 || w == 0) return GS360_OK;
    if (src_stride == 0) src_stride = (size_t)W * C * esize;
    if (dst_stride == 0) dst_stride = (size_t)w * C * esize;
    HIP_TRY(hipSetDevice(c->device));
    Staging& S = c->stage[slot];
    size_t src_bytes = src_stride * (size_t)H, dst_bytes = dst_stride * (size_t)h;
    size_t npx = (size_t)h * w, map_bytes = npx * sizeof(float);
    size_t map_al = (map_bytes + 255) & ~(size_t)255;
    if (int rc = ensure(&S.d_src, &S.src_cap, src_bytes)) return rc;
    if (int rc = ensure(&S.d_dst, &S.dst_cap, dst_bytes)) return rc;
    if (int rc = ensure(&S.d_aux, &S.aux_cap, 2 * map_al + npx)) return rc;
    hipStream_t st = c->stream[slot];
    float* dmx = (float*)S.d_aux;
    float* dmy = (float*)((uint8_t*)S.d_aux + map_al);
    uint8_t* dva = (uint8_t*)S.d_aux + 2 * map_al;
    HIP_TRY(hipMemcpyAsync(S.d_src, src, src_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dmx, map_x, map_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dmy, map_y, map_bytes, hipMemcpyHostToDevice, st));
    if (valid) HIP_TRY(hipMemcpyAsync(dva, valid, npx, hipMemcpyHostToDevice, st));
    if (int rc = (esize == 2 ? gs360_remap_table_u16 : gs360_remap_table_u8)(c, S.d_src, H, W, C, src_stride, dmx, dmy, valid ? dva : nullptr,
                                                                             h, w, interp, border_value, fill_value, S.d_dst, dst_stride, slot))
        return rc;
    HIP_TRY(hipMemcpyAsync(dst, S.d_dst, dst_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return GS360_OK;
}

}  // namespace

void gs360::build_cubic_table(int16_t* out) {
    float c1[32 * 4];
    cubic_coef1d(c1);
    build_tab2d(c1, 4, out);
}

void gs360::build_lanczos4_table(int16_t* out) {
    float c1[32 * 8];
    lanczos4_coef1d(c1);
    build_tab2d(c1, 8, out);
}

// float32 1-D phase tables of the CV_16U samplers: [0,64) linear (1-x, x), [64,192) cubic, [192,448) lanczos4
void gs360::build_coef1d(float* out) {
    for (int i = 0; i < 32; ++i) {
        const float x = (float)i * (1.0f / 32.0f);
        out[i * 2] = 1.f - x;
        out[i * 2 + 1] = x;
    }
    cubic_coef1d(out + 64);
    lanczos4_coef1d(out + 192);
}

int gs360_map_plan_create(gs360_ctx* c, const float* map_x, const float* map_y, const uint8_t* valid, int h, int w,
                          int nearest, int slot, gs360_map_plan** out) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    if (!map_x || !map_y || !out) return fail(GS360_ERR_ARG, "NULL argument");
    if (h < 1 || w < 1 || h >= 32767 || w >= 32767) return fail(GS360_ERR_ARG, "bad map size %dx%d", w, h);
    HIP_TRY(hipSetDevice(c->device));
    gs360_map_plan* p = new (std::nothrow) gs360_map_plan();
    if (!p) return fail(GS360_ERR_NOMEM, "out of host memory");
    p->device = c->device; p->h = h; p->w = w; p->nearest = nearest ? 1 : 0; p->has_valid = valid ? 1 : 0;
    const size_t n = (size_t)h * (size_t)w;
    hipError_t e = hipMalloc((void**)&p->d_packed, n * sizeof(uint32_t) + kSlack);
    if (e == hipSuccess) e = hipMalloc((void**)&p->d_hi, n + kSlack);
    if (e == hipSuccess) e = launch_map_pack(map_x, map_y, valid, (int64_t)n, p->nearest, p->d_packed, p->d_hi, c->stream[slot]);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream[slot]);      // the caller may release its maps on return
    if (e != hipSuccess) {
        if (p->d_packed) (void)hipFree(p->d_packed);
        if (p->d_hi) (void)hipFree(p->d_hi);
        delete p;
        return fail(e == hipErrorOutOfMemory ? GS360_ERR_NOMEM : GS360_ERR_HIP, "map plan setup failed: %s", hipGetErrorString(e));
    }
    *out = p;
    return GS360_OK;
}

int gs360_map_plan_destroy(gs360_ctx* c, gs360_map_plan* p) {
    if (!c) return fail(GS360_ERR_ARG, "ctx is NULL");
    if (!p) return GS360_OK;
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipDeviceSynchronize());
    if (p->d_packed) HIP_TRY(hipFree(p->d_packed));
    if (p->d_hi) HIP_TRY(hipFree(p->d_hi));
    for (gs360::TsPlan* t : p->ts_plans) gs360::ts_plan_free(t);
    delete p;
    return GS360_OK;
}

int gs360_remap_tables_u8(gs360_ctx* c, const gs360_remap_job* jobs, int n_jobs, int C, int interp,
                          const double* border_value, int slot) {
    return remap_batches(c, jobs, nullptr, n_jobs, C, interp, border_value, slot, 1);
}

int gs360_remap_plans_u8(gs360_ctx* c, const gs360_remap_job* jobs, const gs360_map_plan* const* plans, int n_jobs, int C,
                         int interp, const double* border_value, int slot) {
    if (n_jobs > 0 && !plans) return fail(GS360_ERR_ARG, "plans is NULL");
    return remap_batches(c, jobs, plans, n_jobs, C, interp, border_value, slot, 1);
}

int gs360_remap_tables_u16(gs360_ctx* c, const gs360_remap_job* jobs, int n_jobs, int C, int interp,
                           const double* border_value, int slot) {
    return remap_batches(c, jobs, nullptr, n_jobs, C, interp, border_value, slot, 2);
}

int gs360_remap_plans_u16(gs360_ctx* c, const gs360_remap_job* jobs, const gs360_map_plan* const* plans, int n_jobs, int C,
                          int interp, const double* border_value, int slot) {
    if (n_jobs > 0 && !plans) return fail(GS360_ERR_ARG, "plans is NULL");
    return remap_batches(c, jobs, plans, n_jobs, C, interp, border_value, slot, 2);
}

int gs360_remap_table_u8(gs360_ctx* c, const void* src, int H, int W, int C, size_t src_stride, const float* map_x,
                         const float* map_y, const uint8_t* valid, int h, int w, int interp,
                         const double* border_value, int fill_value, void* dst, size_t dst_stride, int slot) {
    const gs360_remap_job J = one_job(src, H, W, src_stride, map_x, map_y, valid, h, w, fill_value, dst, dst_stride);
    return gs360_remap_tables_u8(c, &J, 1, C, interp, border_value, slot);
}

int gs360_remap_table_u16(gs360_ctx* c, const void* src, int H, int W, int C, size_t src_stride, const float* map_x,
                          const float* map_y, const uint8_t* valid, int h, int w, int interp,
                          const double* border_value, int fill_value, void* dst, size_t dst_stride, int slot) {
    const gs360_remap_job J = one_job(src, H, W, src_stride, map_x, map_y, valid, h, w, fill_value, dst, dst_stride);
    return gs360_remap_tables_u16(c, &J, 1, C, interp, border_value, slot);
}

// ---- fused fisheye -> views --------------------------------------------------------------------
int gs360_fisheye_views_border_u8(gs360_ctx* c, const void* const* src_lens, const gs360_calib* calibs, int C, size_t src_stride,
                                  const gs360_view* views, int n_views, double lens_fov_deg, int interp, int mask_outside,
                                  int mask_value, const double* border_value, void* const* dst, size_t dst_stride,
                                  uint8_t* const* valid_out, int slot) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    if (!src_lens || !calibs || !views || !dst) return fail(GS360_ERR_ARG, "NULL argument");
    if (n_views < 0) return fail(GS360_ERR_ARG, "negative count");
    if (n_views == 0) return GS360_OK;
    if (int rc = check_channels(C)) return rc;
    if (int rc = check_table_interp(interp)) return rc;
    for (int k = 0; k < n_views; ++k) {
        if (!src_lens[k] || !dst[k]) return fail(GS360_ERR_ARG, "NULL image pointer for view %d", k);
        if (calibs[k].width < 1 || calibs[k].height < 1 || calibs[k].width >= 32767 || calibs[k].height >= 32767)
            return fail(GS360_ERR_ARG, "bad sensor size for view %d", k);
        if (calibs[k].width != calibs[0].width && src_stride != 0)
            return fail(GS360_ERR_ARG, "explicit src_stride needs equal sensor widths");
        if (views[k].width < 1 || views[k].height < 1 || views[k].width > 32768 || views[k].height > 32768)
            return fail(GS360_ERR_ARG, "view %d has bad size", k);
    }
    // (a launch keeps a single src_stride in its parameter block; refused before the first launch so that no view is written)
    for (int k = 0; k < n_views; ++k)
        if (calibs[k].width != calibs[k - k % GS360_MAX_VIEWS].width)
            return fail(GS360_ERR_UNSUPPORTED, "views of one call must share the sensor width");
    HIP_TRY(hipSetDevice(c->device));
    mask_value = mask_value < 0 ? 0 : (mask_value > 255 ? 255 : mask_value);
    for (int v0 = 0; v0 < n_views; v0 += GS360_MAX_VIEWS) {
        int nv = n_views - v0 < GS360_MAX_VIEWS ? n_views - v0 : GS360_MAX_VIEWS;
        FeBatch B;
        std::memset(&B, 0, sizeof(B));
        FeCommon& L = B.common;
        int base = 0;
        for (int k = 0; k < nv; ++k) {
            make_fe_view(calibs[v0 + k], views[v0 + k], lens_fov_deg, &B.view[k]);
            B.view[k].src = (const uint8_t*)src_lens[v0 + k];
            B.view[k].dst = (uint8_t*)dst[v0 + k];
            B.view[k].valid_out = valid_out ? valid_out[v0 + k] : nullptr;
            B.view[k].tile_base = base;
            base += B.view[k].tiles_x * B.view[k].tiles_y;
        }
        L.n_views = nv;
        L.total_tiles = base;
        L.chunk = (base + 7) / 8;
        L.interp = interp; L.mask_outside = mask_outside ? 1 : 0; L.mask_value = mask_value;
        L.src_stride = (int64_t)(src_stride ? src_stride : (size_t)calibs[v0].width * C);
        L.dst_stride = (int64_t)dst_stride;
        for (int k = 0; k < 4; ++k) L.cval[k] = sat_u8(border_value ? border_value[k] : 0.0);
        L.cubic_tab = interp == GS360_INTERP_LANCZOS4 ? c->d_lanczos : c->d_cubic;
        L.pipelined = 1;
        for (int k = 0; k < nv; ++k)
            if (calibs[v0 + k].width < 8 || (uint64_t)L.src_stride * (uint64_t)calibs[v0 + k].height >= ((uint64_t)1 << 32)) L.pipelined = 0;
        // (a 3-channel image off a dword boundary: the pipelined gathers read whole dwords from the base on; the straight-line samplers do not)
        for (int k = 0; k < nv && C == 3; ++k)
            if (reinterpret_cast<uintptr_t>(src_lens[v0 + k]) & 3) L.pipelined = 0;
        if ((uint64_t)L.src_stride >= ((uint64_t)1 << 24)) L.pipelined = 0;
        int persist_blocks = c->prop.multiProcessorCount * 8;
        if (const int v = opt(c, kOptTablePersist); v >= 0) persist_blocks = v;
        HIP_TRY(launch_fisheye(B, persist_blocks, C, c->stream[slot]));
    }
    return GS360_OK;
}

// borderValue=float(mask_value) -> Scalar(v,0,0,0), DF:2007: the value on channel 0 of the image as it lies in memory
int gs360_fisheye_views_u8(gs360_ctx* c, const void* const* src_lens, const gs360_calib* calibs, int C, size_t src_stride,
                           const gs360_view* views, int n_views, double lens_fov_deg, int interp, int mask_outside,
                           int mask_value, void* const* dst, size_t dst_stride, uint8_t* const* valid_out, int slot) {
    const double border[4] = {(double)mask_value, 0.0, 0.0, 0.0};      // (saturated to 0..255 like the mask value itself)
    return gs360_fisheye_views_border_u8(c, src_lens, calibs, C, src_stride, views, n_views, lens_fov_deg, interp, mask_outside,
                                         mask_value, border, dst, dst_stride, valid_out, slot);
}

// ---- host-buffer conveniences ------------------------------------------------------------------
int gs360_remap_table_u8_host(gs360_ctx* c, const uint8_t* src, int H, int W, int C, size_t src_stride, const float* map_x,
                              const float* map_y, const uint8_t* valid, int h, int w, int interp,
                              const double* border_value, int fill_value, uint8_t* dst, size_t dst_stride, int slot) {
    return remap_table_host_impl(c, src, H, W, C, src_stride, map_x, map_y, valid, h, w, interp, border_value, fill_value, dst, dst_stride, slot, 1);
}
int gs360_remap_table_u16_host(gs360_ctx* c, const uint16_t* src, int H, int W, int C, size_t src_stride, const float* map_x,
                               const float* map_y, const uint8_t* valid, int h, int w, int interp,
                               const double* border_value, int fill_value, uint16_t* dst, size_t dst_stride, int slot) {
    return remap_table_host_impl(c, src, H, W, C, src_stride, map_x, map_y, valid, h, w, interp, border_value, fill_value, dst, dst_stride, slot, 2);
}
