// gs360_capi_equirect.hip -- C-ABI glue of equirect -> views (include/gs360.h): EQ-SPEC per-view constants, the kernel choice
// (source-major, LDS-staged or gather), yaw-ring grouping, the u8 / u16 / masked_u8 entry points and their host conveniences.
#include "gs360_capi_internal.h"

using namespace gs360;

namespace {
constexpr size_t kSmLdsPerGroup = 80 * 1024;   // two workgroups of the source-major kernel per CU (160 KiB of LDS)
constexpr double kSmMinPixels = 3.5e6;           // automatic selection of the source-major kernel: output pixels of the call (smaller calls are launch-bound)
constexpr int kSmFamilyMinFrames = 4;          // automatic selection of the source-major kernel for calls of several rings: frames per call ...
constexpr int kSmMaxBoxPct = 160;              // ... and tile boxes at most this large relative to their grid cells (profiles/r05/srcmajor_family_sweep.txt)
static_assert(sizeof(EqLaunch) <= 4096, "EqLaunch travels as a kernel argument");

// Source texels stepped per output pixel at the view centre.
double source_step(const gs360_view& v, int W) {
    const double hf = clampd(v.hfov_deg, 1e-3, 179.9) * kPi / 180.0;
    return (double)W / (2.0 * kPi) * 2.0 * std::tan(hf * 0.5) / (double)v.width;
}

// EQ-SPEC v1 per-view constants.  Convention: gs360_GUI.py:377-395 / :419-424 of the reference.
void make_eq_view(const gs360_view& v, int W, bool fisheye_out, int lanemap, EqView* o) {
    double hf = clampd(v.hfov_deg, 1e-3, 179.9) * kPi / 180.0;
    double vf = clampd(v.vfov_deg, 1e-3, 179.9) * kPi / 180.0;
    o->sxu = (float)(std::tan(hf * 0.5) / (double)v.width);
    o->syv = (float)(std::tan(vf * 0.5) / (double)v.height);
    double pitch = v.pitch_deg * kPi / 180.0;
    o->sp = (float)std::sin(pitch);
    o->cp = (float)std::cos(pitch);
    double x0 = (v.yaw_deg / 360.0 + 0.5) * (double)W - 0.5;
    double fl = std::floor(x0);
    o->x0f32 = (float)(32.0 * (x0 - fl));
    long xi = (long)fl % (long)W;
    if (xi < 0) xi += W;
    o->x0i32 = (int32_t)(32 * xi);
    o->out_w = v.width;
    o->out_h = v.height;
    // The kernel computes the left half of every row and mirrors it; level views also mirror top/bottom.
    o->level = (o->sp == 0.0f && o->cp == 1.0f) ? 1 : 0;
    // Lane map (gs360_kernels.hip): source pixels stepped per output pixel at the view centre.  Above ~3 the view
    // bends across so many source rows per 64-pixel output row that compact 4x16 gather patches touch fewer cache
    // lines (cfg2: 4.6 -> blocked, -3 %); below it full rows coalesce better and need less arithmetic (cfg1 1.7,
    // cfg3 2.0, cfg5 1.25: blocked would cost 7-19 %).  GS360_LANEMAP=rows|blocked overrides (tests, probes).
    const double step = source_step(v, W);
    o->blocked = step >= 3.0 ? 1 : 0;
    if (lanemap >= 0) o->blocked = lanemap;           // option "lanemap": tests, probes
    o->fish = 0;
    if (fisheye_out) {   // image-plane radius 1 <-> 90 degrees off axis; hfov/vfov = full field of view of the fisheye image
        o->fish = 1;
        o->sxu = (float)(clampd(v.hfov_deg, 1e-3, 360.0) / 180.0 / (double)v.width);
        o->syv = (float)(clampd(v.vfov_deg, 1e-3, 360.0) / 180.0 / (double)v.height);
        o->level = 0;
        o->blocked = 0;
        o->tiles_y = (v.height + kTileH - 1) / kTileH;
    }
    const int half_w = (v.width + 1) / 2;
    o->tiles_x = (half_w + kTileW - 1) / kTileW;
    o->tiles_y = o->level ? ((v.height + 1) / 2 + kTileH / 2 - 1) / (kTileH / 2) : (v.height + kTileH - 1) / kTileH;
}

struct EqCall {                 // the arguments of one equirect call (defaults of the strides resolved by validate_equirect_call)
    gs360_ctx* c;
    const void* const* src_frames; const void* const* mask_frames;
    int n_frames, W, H, C;
    size_t src_stride, mask_stride;
    const gs360_view* views; int n_views;
    void* const* dst; size_t dst_stride;
    int interp; uint32_t flags; int slot, esize;
    int mask_pitch_dw; size_t mask_bits_bytes;   // dwords per row / bytes per frame of the keep-bit images
};

// 1: an empty batch (a no-op); otherwise 0 or an error code.
int validate_equirect_call(EqCall& q) {
    if (int rc = check_ctx_slot(q.c, q.slot)) return rc;
    if (!q.src_frames || !q.views || !q.dst) return fail(GS360_ERR_ARG, "NULL argument");
    const int W = q.W, H = q.H, C = q.C, esize = q.esize;
    if (q.mask_frames) {
        if (q.mask_stride == 0) q.mask_stride = (size_t)W;
        if (q.mask_stride < (size_t)W) return fail(GS360_ERR_ARG, "mask_stride smaller than a row");
        if ((uint64_t)q.mask_stride * (uint64_t)H >= ((uint64_t)1 << 32)) return fail(GS360_ERR_UNSUPPORTED, "mask too large");
        if (H + 1 > 65535) return fail(GS360_ERR_UNSUPPORTED, "masked equirect calls take H < 65535 (the mask pack pass launches one grid row per mask row)");
        for (int f = 0; f < q.n_frames; ++f)
            if (!q.mask_frames[f]) return fail(GS360_ERR_ARG, "mask_frames[%d] is NULL", f);
    }
    if (q.n_frames < 0 || q.n_views < 0) return fail(GS360_ERR_ARG, "negative count");
    if (q.n_frames == 0 || q.n_views == 0) return 1;
    if (int rc = check_channels(C)) return rc;
    if (W < 8 || H < 2 || W > (1 << 21) || H > (1 << 21))
        return fail(GS360_ERR_ARG, "bad source size %dx%d (an equirect frame is at least 8 texels wide)", W, H);
    // the kernels form a flipped ring member's latitude with v_mad_i32_i24 (24-bit operands): 32 H must stay below 2^23
    if (H >= (1 << 18)) return fail(GS360_ERR_UNSUPPORTED, "source height %d: the equirect kernels take H < 262144", H);
    if (q.interp != GS360_INTERP_LINEAR && q.interp != GS360_INTERP_CUBIC)
        return fail(GS360_ERR_UNSUPPORTED, "equirect path implements INTER_LINEAR (1) and INTER_CUBIC (2), got %d", q.interp);
    if (q.flags & ~(uint32_t)GS360_EQ_FISHEYE_OUT) return fail(GS360_ERR_ARG, "unknown flags 0x%x", q.flags);
    if (q.src_stride == 0) q.src_stride = (size_t)W * C * esize;
    if (q.src_stride < (size_t)W * C * esize) return fail(GS360_ERR_ARG, "src_stride smaller than a row");
    if (esize == 2 && ((q.src_stride | q.dst_stride) & 1)) return fail(GS360_ERR_ARG, "16-bit images need even strides");
    if (q.src_stride >= ((size_t)1 << 24) || (uint64_t)q.src_stride * (uint64_t)H >= ((uint64_t)1 << 32))
        return fail(GS360_ERR_UNSUPPORTED, "frame too large for 32-bit tap offsets (stride %zu x %d rows)", q.src_stride, H);
    for (int k = 0; k < q.n_views; ++k) {
        const gs360_view& v = q.views[k];
        if (v.width < 1 || v.height < 1 || v.width > 32768 || v.height > 32768)
            return fail(GS360_ERR_ARG, "view %d has bad size %dx%d", k, v.width, v.height);
        if (q.dst_stride && q.dst_stride < (size_t)v.width * C * esize) return fail(GS360_ERR_ARG, "dst_stride smaller than a row");
        if (!std::isfinite(v.yaw_deg) || !std::isfinite(v.pitch_deg) || !std::isfinite(v.hfov_deg) || !std::isfinite(v.vfov_deg))
            return fail(GS360_ERR_ARG, "view %d has a non-finite angle", k);
    }
    for (int f = 0; f < q.n_frames; ++f) {
        if (!q.src_frames[f]) return fail(GS360_ERR_ARG, "src_frames[%d] is NULL", f);
        if (C == 3 && esize == 1 && ((uintptr_t)q.src_frames[f] & 3))
            return fail(GS360_ERR_ARG, "src_frames[%d] must be 4-byte aligned (the RGB tap reads are dword-aligned)", f);
    }
    for (int i = 0; i < q.n_frames * q.n_views; ++i)
        if (!q.dst[i]) return fail(GS360_ERR_ARG, "dst[%d] is NULL", i);
    return 0;
}

// The fields every launch of the call shares, and the sources and destinations of frames [f0, f0 + nf): the launch's view k is the
// call's view order[k] (order NULL: view k).
void fill_eq_common(EqLaunch& L, const EqCall& q, int f0, int nf, const int* order, int nv) {
    for (int f = 0; f < nf; ++f) {
        L.src[f] = (const uint8_t*)q.src_frames[f0 + f];
        for (int k = 0; k < nv; ++k) L.dst[f * nv + k] = (uint8_t*)q.dst[(size_t)(f0 + f) * q.n_views + (order ? order[k] : k)];
    }
    L.kx32 = (float)(32.0 * (double)q.W / (2.0 * kPi));
    L.ky32 = (float)(32.0 * (double)q.H / kPi);
    L.W = q.W; L.H = q.H;
    L.y0i32 = 16 * q.H - 16;
    L.n_views = nv; L.n_frames = nf;
    L.src_stride = (int64_t)q.src_stride; L.dst_stride = (int64_t)q.dst_stride;
}

// keep-masks: thresholded once per launch into bit images (the kernels only test `< 128`), behind the caller's upload on the launch
// stream: a streaming pass over W x H bytes per frame, ~7 us for an 8K mask.  (The previous launch on this stream may still read the
// images: a reallocation's hipFree synchronises the device.)
int pack_masks(const EqCall& q, int f0, int nf) {
    Staging& st = q.c->stage[q.slot];
    if (int rc = ensure(&st.d_maskbits, &st.maskbits_cap, q.mask_bits_bytes * (size_t)nf)) return rc;
    MaskPack P;
    std::memset(&P, 0, sizeof(P));
    for (int f = 0; f < nf; ++f) {
        P.src[f] = (const uint8_t*)q.mask_frames[f0 + f];
        P.dst[f] = (uint32_t*)((uint8_t*)st.d_maskbits + q.mask_bits_bytes * (size_t)f);
    }
    P.W = q.W; P.H = q.H; P.pitch_dw = q.mask_pitch_dw; P.n = nf;
    P.stride = (int64_t)q.mask_stride;
    HIP_TRY(launch_mask_pack(P, q.c->stream[q.slot]));
    return GS360_OK;
}

const uint8_t* mask_bits(const EqCall& q, int f) {   // frame f's keep-bit image of the current frame chunk
    return (const uint8_t*)q.c->stage[q.slot].d_maskbits + q.mask_bits_bytes * (size_t)f;
}

struct SmPlanHold {             // the call's source-major plan, released on every way out
    SmCache& cache;
    SmPlan* plan = nullptr;
    ~SmPlanHold() { sm_release(cache, plan); }
};

constexpr int kSmFellThrough = 1;   // try_srcmajor launched nothing: the gather kernels take the call

// Source-major kernel (gs360_srcmajor.hip): a call whose views are yaw rings of one size filling their circle (`--count N`, PC:794; the
// presets' pitched ring pairs, PC:616-680) streams every source tile once for all views instead of gathering per view.  Where it wins
// (8K sources, N views per ring, s source texels per output pixel):
//   * ONE level ring (profiles/r05/srcmajor_ring_sweep.txt, srcmajor_small_jobs.txt): N >= 6 at every s measured (1.5 .. 4.6) and every
//     number of frames per call -- sixteen frames -8 .. -42 % (cfg2 19.0 -> 14.9 us per frame, cfg1 47.9 -> 33.6), one frame -3 .. -26 %
//     (cfg2 21.7 -> 16.0: what the drop-in engine launches) -- as long as the call has work to fill the GPU (>= 3.5 M output pixels; a
//     4K -> 6 x 400^2 frame is launch-bound either way); N = 5 from s = 2.25 and two frames; N = 4 never (neighbours overlap by a
//     quarter of their field only: +14 .. +44 %);
//   * SEVERAL rings (srcmajor_family_sweep.txt): from four frames per call, eight views and s = 1.75, unless the views reach so close to
//     a pole that the tile boxes outgrow their grid cells (kSmMaxBoxPct).
// Option "srcmajor": 0 never, 1 whenever the geometry fits (tests, probes).  Decided before the ring grouping (which keeps blocked views
// apart); a geometry that does not fit the plan format falls through to the gather kernels.
// Returns GS360_OK (launched), kSmFellThrough or an error code.
int try_srcmajor(const EqCall& q, const std::vector<EqView>& ev) {
    gs360_ctx* c = q.c;
    const int opt_srcmajor = opt(c, kOptSrcMajor);
    const bool fish = (q.flags & GS360_EQ_FISHEYE_OUT) != 0;
    if (!(opt_srcmajor != 0 && q.esize == 1 && q.C == 3 && q.interp == GS360_INTERP_LINEAR && !fish && q.n_views >= 2 &&
          q.n_views <= GS360_MAX_VIEWS))
        return kSmFellThrough;
    bool ring = true;
    SmShape shape;
    std::vector<EqLaunch> Ls;
    for (int f0 = 0; f0 < q.n_frames && ring; f0 += GS360_MAX_FRAMES) {
        const int nf = q.n_frames - f0 < GS360_MAX_FRAMES ? q.n_frames - f0 : GS360_MAX_FRAMES;
        EqLaunch L;
        std::memset(&L, 0, sizeof(L));
        for (int k = 0; k < q.n_views; ++k) L.view[k] = ev[k];
        L.n_rings = 1; L.ring_first[0] = 0; L.ring_count[0] = q.n_views;
        fill_eq_common(L, q, f0, nf, nullptr, q.n_views);
        ring = sm_eligible(L, q.C, q.esize, q.interp, q.mask_frames != nullptr, &shape);     // (the shape depends on the views only: the same for every chunk)
        Ls.push_back(L);
    }
    if (ring && opt_srcmajor < 0) {
        const gs360_view& v = q.views[0];
        const double step = source_step(v, q.W);
        const double out_px = (double)q.n_frames * q.n_views * v.width * v.height;
        if (shape.n_rings == 1) ring = out_px >= kSmMinPixels && (shape.N >= 6 ? step >= 1.5 : shape.N == 5 && q.n_frames >= 2 && step >= 2.25);
        else ring = q.n_frames >= kSmFamilyMinFrames && q.n_views >= 8 && step >= 1.75;
    }
    if (!ring) return kSmFellThrough;
    // the plan is decided ONCE per call (first chunk) and held until the last chunk is launched: a tail chunk of another size must not pick
    // another plan -- or find its plan evicted -- after earlier chunks have rendered
    SmPlanHold hold{c->sm};
    hipError_t he = hipSuccess;
    int seen_box_pct = 0;
    const int rc = sm_prepare(Ls[0], shape, c->sm, q.mask_frames != nullptr, opt(c, kOptSrcMajorBx), opt(c, kOptSrcMajorRows),
                              opt(c, kOptSrcMajorImages), opt(c, kOptSrcMajorAdapt) != 0, opt_srcmajor < 0 ? kSmMaxBoxPct : 0, kSmLdsPerGroup,
                              c->prop.multiProcessorCount, c->stream[q.slot], &he, &hold.plan, &seen_box_pct);
    c->last_sm_box_pct.store(seen_box_pct, std::memory_order_relaxed);
    if (rc < 0) return fail(he == hipErrorOutOfMemory ? GS360_ERR_NOMEM : GS360_ERR_HIP, "source-major plan failed: %s", hipGetErrorString(he));
    if (rc == 1) return kSmFellThrough;          // the geometry does not fit the plan format: the gather kernels (nothing launched yet)
    for (size_t i = 0; i < Ls.size(); ++i) {
        EqLaunch& L = Ls[i];
        if (q.mask_frames) {                     // (packed per chunk of frames: the staging images are reused)
            if (int prc = pack_masks(q, (int)i * GS360_MAX_FRAMES, L.n_frames)) return prc;
            for (int f = 0; f < L.n_frames; ++f) L.mask[f] = mask_bits(q, f);
            L.mask_stride = (int64_t)q.mask_pitch_dw * 4;
        }
        int info[4] = {0, 0, 0, 0};
        const int lrc = sm_launch(L, shape, hold.plan, opt(c, kOptSrcMajorImages), opt(c, kOptSrcMajorStage) != 0, kSmLdsPerGroup,
                                  c->prop.multiProcessorCount, c->stream[q.slot], &he, info);
        c->last_sm_box_pct.store(info[0], std::memory_order_relaxed);
        c->last_sm_rows.store(info[1], std::memory_order_relaxed);
        c->last_sm_images.store(info[2], std::memory_order_relaxed);
        c->last_sm_stage.store(info[3], std::memory_order_relaxed);
        if (lrc < 0) return fail(he == hipErrorOutOfMemory ? GS360_ERR_NOMEM : GS360_ERR_HIP, "source-major launch failed: %s", hipGetErrorString(he));
    }
    c->last_eq_kernel.store(2, std::memory_order_relaxed);
    return GS360_OK;
}

// LDS-staged kernel (eq_staged_kernel, north_star's "LDS-staged source texels"): bilinear RGB u8 views whose row stride keeps dword
// alignment from row to row; its wavefront tiles are 16 x 16 pixels of the general (non-level) tiling.  When it is taken
// (steady-state clocks, profiles/r04/stage_sweep.txt, settle_ab.txt, stage_auto_ab.txt): the gather form of PITCHED views that step
// >= 1.75 source texels per output pixel at their centre is bound by the texture-address path, and staging wins there (8K ->
// full360coverage: -2 % at step 1.75, -8 % at 1.96, -14 % at 2.6); level views keep the gather kernels' horizon sharing (an all-level
// ring: level at step 2, -6 % at 2.6; cfg1 36.6 vs 44.3 us staged) and below 1.75 the arithmetic decides (cfg5 75.2 vs 88.7).
// Splitting a call into a staged and a gather launch loses more in launch tails than it wins (cfg3 95.8 us against 84.4 all
// gathered and 78.4 all staged), so the CALL is staged as a whole when such views write most of its pixels: its views get blocked = 2.
// GS360_STAGE=0: never; GS360_STAGE=1: every call that can (tests, probes).
void apply_staged_rule(const EqCall& q, std::vector<EqView>& ev) {
    const int mode = opt(q.c, kOptStage);                 // -1 auto
    // (the staged kernel forms destination row offsets in 32 bits with a 24-bit multiply: padded strides beyond that take the gather kernels)
    bool can = mode != 0 && q.C == 3 && q.esize == 1 && q.interp == GS360_INTERP_LINEAR && (q.src_stride & 3) == 0 &&
               q.dst_stride < ((size_t)1 << 24);
    double px_all = 0.0, px_win = 0.0;
    for (int k = 0; k < q.n_views && can; ++k) {
        const gs360_view& v = q.views[k];
        can = ev[k].blocked == 0;
        const double step = source_step(v, q.W);
        const double px = (double)v.width * (double)v.height;
        px_all += px;
        // (views whose rows are not whole dwords: the staged kernel would write them byte by byte, the gather kernels have a dword path)
        const size_t row_bytes = q.dst_stride ? q.dst_stride : (size_t)v.width * 3;
        if ((uint64_t)v.height * (uint64_t)row_bytes >= ((uint64_t)1 << 32)) can = false;
        if (!ev[k].level && !ev[k].fish && step >= 1.75 && (row_bytes & 3) == 0 && (v.width & 3) == 0) px_win += px;
    }
    if (can && (mode == 1 || 2.0 * px_win > px_all))
        for (EqView& e : ev) {
            e.blocked = 2;
            e.level = 0;
            e.tiles_y = (e.out_h + kTileH - 1) / kTileH;
        }
}

// Yaw rings: views whose EQ-SPEC constants agree in everything but the integer longitude offset x0i32 -- and possibly the sign of the
// pitch -- form a ring: the kernel evaluates a tile's coordinates once and samples it for every member (the presets' yaw steps are whole
// texels: `yaw = i * 360 / count`, PC:794).  Float equality of the rounded constants is the criterion, so the grouping can never change
// a result.  Sets every view's `flip`; returns the rings (view indices), gather rings first, then staged ones.
std::vector<std::vector<int>> group_rings(const EqCall& q, std::vector<EqView>& ev) {
    // Ring size: unlimited for the row-per-slot lane map (arithmetic-bound views: cfg3 119 -> 99 -> 95 -> 93 us per frame for
    // rings of 1 / 2 / 3 / 4-8 views).  Views on the blocked lane map are memory-bound and gain nothing from shared arithmetic,
    // while a workgroup that walks six views in a row lengthens the launch's tail (cfg2 20.3 -> 22.6 us per frame): no sharing.
    const int opt_ring = opt(q.c, kOptRing);
    int ring_max = GS360_MAX_VIEWS, ring_max_blocked = 1;
    if (opt_ring >= 1) ring_max = ring_max_blocked = opt_ring;      // option "ring" (tests / probes): 1 = no sharing anywhere, n = at most n views per ring
    std::vector<std::vector<int>> rings;
    const bool ring_forced = opt_ring >= 1;
    for (;;) {
        rings.clear();
        for (int k = 0; k < q.n_views; ++k) {
            const EqView& b = ev[k];
            int hit = -1;
            for (size_t r = 0; r < rings.size() && hit < 0; ++r) {
                const EqView& a = ev[rings[r][0]];
                if ((int)rings[r].size() < (b.blocked == 1 ? ring_max_blocked : ring_max) && a.sxu == b.sxu && a.syv == b.syv && a.cp == b.cp && (a.sp == b.sp || a.sp == -b.sp) &&
                    a.x0f32 == b.x0f32 && a.out_w == b.out_w && a.out_h == b.out_h && a.level == b.level && a.fish == b.fish &&
                    a.blocked == b.blocked)
                    hit = (int)r;
            }
            if (hit < 0) { rings.emplace_back(); hit = (int)rings.size() - 1; }
            rings[hit].push_back(k);
            ev[k].flip = ev[rings[hit][0]].sp != b.sp ? 1 : 0;
        }
        // A ring's workgroup walks all its members, so a SMALL job in long rings is too few workgroups to fill the chip twice over
        // (one 5.7K frame -> `default`: one ring of 8 = 1300 workgroups for 1280 resident slots: 61 us against 56 us as two rings of
        // 4; the engine's product path launches one frame at a time).  Halve the ring cap until the job has two rounds of workgroups.
        size_t longest = 1;
        long long wgs = 0;
        for (const auto& r : rings) {
            longest = r.size() > longest ? r.size() : longest;
            wgs += (long long)ev[r[0]].tiles_x * ev[r[0]].tiles_y;
        }
        wgs *= q.n_frames < GS360_MAX_FRAMES ? q.n_frames : GS360_MAX_FRAMES;
        const long long two_rounds = 2ll * q.c->prop.multiProcessorCount * 5;
        if (ring_forced || wgs >= two_rounds || longest <= 2 || ring_max <= 2) break;
        ring_max = (int)((longest + 1) / 2);
    }
    // members with the ring's own pitch sign first, the upside-down ones behind them: the kernel's member loop re-derives its
    // latitude-dependent row offsets once per change of sign (results do not depend on the order)
    for (auto& r : rings) std::stable_partition(r.begin(), r.end(), [&](int k) { return ev[k].flip == 0; });
    std::stable_partition(rings.begin(), rings.end(), [&](const std::vector<int>& r) { return ev[r[0]].blocked != 2; });   // gather rings, then staged ones
    return rings;
}

// Consecutive rings of one kind (staged or gather) share a launch while their views fit GS360_MAX_VIEWS; one launch per chunk of frames.
int launch_ring_groups(const EqCall& q, const std::vector<EqView>& ev, const std::vector<std::vector<int>>& rings) {
    gs360_ctx* c = q.c;
    const int opt_xcd = opt(c, kOptXcdGroup);
    size_t r0 = 0;
    while (r0 < rings.size()) {
        size_t r1 = r0;
        int nv = 0;
        const bool staged = ev[rings[r0][0]].blocked == 2;          // staged rings and gather rings never share a launch
        while (r1 < rings.size() && nv + (int)rings[r1].size() <= GS360_MAX_VIEWS && (ev[rings[r1][0]].blocked == 2) == staged)
            nv += (int)rings[r1++].size();
        for (int f0 = 0; f0 < q.n_frames; f0 += GS360_MAX_FRAMES) {
            int nf = q.n_frames - f0 < GS360_MAX_FRAMES ? q.n_frames - f0 : GS360_MAX_FRAMES;
            EqLaunch L;
            std::memset(&L, 0, sizeof(L));
            int order[GS360_MAX_VIEWS];
            int base = 0, j = 0;
            for (size_t r = r0; r < r1; ++r) {
                const EqView& lead = ev[rings[r][0]];
                L.ring_first[r - r0] = j;
                L.ring_count[r - r0] = (int32_t)rings[r].size();
                for (int idx : rings[r]) {
                    L.view[j] = ev[idx];
                    L.view[j].tile_base = base;
                    order[j++] = idx;
                }
                base += lead.tiles_x * lead.tiles_y;
            }
            L.n_rings = (int)(r1 - r0);
            // tiles of rings with different member counts differ in cost: deal them to the XCDs in short runs instead of chunks
            L.xcd_group_log2 = -1;
            for (size_t r = r0; r < r1; ++r)
                if (rings[r].size() != rings[r0].size()) L.xcd_group_log2 = 5;
            if (opt_xcd >= -1) L.xcd_group_log2 = opt_xcd;          // option "xcd_group" (probes): -1 = chunks, g = runs of 2^g tiles
            // Persistent workgroups for the cubic variants (one LDS weight-table fill per workgroup instead of per tile) are OFF:
            // an equirect tile already spreads the fill over its mirrored halves and ring members (2048-32768 pixels), and the
            // static walk costs more in balance than the fill saves (cfg2 / cfg1 / cfg3 cubic: 33.4 / 86.5 / 161.5 us per frame
            // with one tile per workgroup, 35.5 / 90.2 / 177.5 with 2048 persistent ones; profiles/r03/persistent_cubic_ab.txt).
            // The cv2 table kernel, 1024 pixels per tile, gains 12 % from it (launch_table_batch).
            L.persist_blocks = opt(c, kOptEqPersist);      // option "eq_persist" (probes): grid cap
            if (q.mask_frames && (r0 == 0 || q.n_frames > GS360_MAX_FRAMES))   // (one frame chunk: later ring groups reuse the images)
                if (int rc = pack_masks(q, f0, nf)) return rc;
            fill_eq_common(L, q, f0, nf, order, nv);
            if (q.mask_frames)
                for (int f = 0; f < nf; ++f) L.mask[f] = mask_bits(q, f);
            L.tiles_per_frame = base;
            L.total_tiles = base * nf;
            L.chunk = (L.total_tiles + 7) / 8;
            L.mask_stride = (int64_t)q.mask_pitch_dw * 4;      // of the bit images
            L.cubic_tab = c->d_cubic;
            HIP_TRY(launch_equirect(L, q.C, q.esize, q.interp == GS360_INTERP_CUBIC, staged, c->stream[q.slot]));
            c->last_eq_kernel.store(staged ? 1 : 0, std::memory_order_relaxed);
        }
        r0 = r1;
    }
    return GS360_OK;
}

int equirect_views_impl(gs360_ctx* c, const void* const* src_frames, const void* const* mask_frames, int n_frames,
                        int W, int H, int C, size_t src_stride, size_t mask_stride, const gs360_view* views,
                        int n_views, void* const* dst, size_t dst_stride, int interp, uint32_t flags, int slot, int esize) {
    EqCall q{c, src_frames, mask_frames, n_frames, W, H, C, src_stride, mask_stride, views, n_views, dst, dst_stride, interp, flags, slot,
             esize, 0, 0};
    if (int rc = validate_equirect_call(q)) return rc < 0 ? rc : GS360_OK;   // (an empty batch is a no-op)
    HIP_TRY(hipSetDevice(c->device));
    q.mask_pitch_dw = (W + 1 + 31) / 32;
    q.mask_bits_bytes = (size_t)q.mask_pitch_dw * 4 * (size_t)(H + 1);
    try {
        const bool fish = (flags & GS360_EQ_FISHEYE_OUT) != 0;
        const int opt_lanemap = opt(c, kOptLanemap);
        std::vector<EqView> ev((size_t)n_views);
        for (int k = 0; k < n_views; ++k) {
            make_eq_view(views[k], W, fish, opt_lanemap, &ev[k]);
            ev[k].flip = 0;
            if (esize == 2) ev[k].blocked = 0;   // 16-bit samples: row-per-slot lane map only
        }
        if (int rc = try_srcmajor(q, ev); rc != kSmFellThrough) return rc;
        apply_staged_rule(q, ev);
        return launch_ring_groups(q, ev, group_rings(q, ev));
    } catch (const std::bad_alloc&) {
        return fail(GS360_ERR_NOMEM, "out of host memory while planning %d views", n_views);
    }
}

int equirect_views_host_impl(gs360_ctx* c, const void* src, int W, int H, int C, size_t src_stride,
                             const gs360_view* views, int n_views, void* const* dst, size_t dst_stride,
                             int interp, uint32_t flags, int slot, int esize) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    if (!src || !views || !dst) return fail(GS360_ERR_ARG, "NULL argument");
    if (n_views <= 0) return n_views == 0 ? GS360_OK : fail(GS360_ERR_ARG, "negative count");
    if (int rc = check_channels(C)) return rc;
    if (W < 2 || H < 2) return fail(GS360_ERR_ARG, "bad source size");
    if (src_stride == 0) src_stride = (size_t)W * C * esize;
    HIP_TRY(hipSetDevice(c->device));
    Staging& S = c->stage[slot];
    size_t src_bytes = src_stride * (size_t)H;
    std::vector<size_t> off(n_views);
    size_t total = 0;
    for (int k = 0; k < n_views; ++k) {
        if (views[k].width < 1 || views[k].height < 1) return fail(GS360_ERR_ARG, "view %d has bad size", k);
        size_t ds = dst_stride ? dst_stride : (size_t)views[k].width * C * esize;
        off[k] = total;
        total += (ds * (size_t)views[k].height + 255) & ~(size_t)255;
    }
    if (int rc = ensure(&S.d_src, &S.src_cap, src_bytes)) return rc;
    if (int rc = ensure(&S.d_dst, &S.dst_cap, total)) return rc;
    hipStream_t st = c->stream[slot];
    HIP_TRY(hipMemcpyAsync(S.d_src, src, src_bytes, hipMemcpyHostToDevice, st));
    std::vector<void*> dptr(n_views);
    for (int k = 0; k < n_views; ++k) dptr[k] = (uint8_t*)S.d_dst + off[k];
    const void* frames[1] = {S.d_src};
    if (int rc = equirect_views_impl(c, frames, nullptr, 1, W, H, C, src_stride, 0, views, n_views, dptr.data(), dst_stride, interp,
                                     flags, slot, esize))
        return rc;
    for (int k = 0; k < n_views; ++k) {
        if (!dst[k]) return fail(GS360_ERR_ARG, "dst[%d] is NULL", k);
        size_t ds = dst_stride ? dst_stride : (size_t)views[k].width * C * esize;
        HIP_TRY(hipMemcpyAsync(dst[k], dptr[k], ds * (size_t)views[k].height, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return GS360_OK;
}

}  // namespace

int gs360_equirect_views_u8(gs360_ctx* c, const void* const* src_frames, int n_frames, int W, int H, int C,
                            size_t src_stride, const gs360_view* views, int n_views, void* const* dst,
                            size_t dst_stride, int interp, uint32_t flags, int slot) {
    return equirect_views_impl(c, src_frames, nullptr, n_frames, W, H, C, src_stride, 0, views, n_views, dst,
                               dst_stride, interp, flags, slot, 1);
}

int gs360_equirect_views_u16(gs360_ctx* c, const void* const* src_frames, int n_frames, int W, int H, int C,
                             size_t src_stride, const gs360_view* views, int n_views, void* const* dst,
                             size_t dst_stride, int interp, uint32_t flags, int slot) {
    return equirect_views_impl(c, src_frames, nullptr, n_frames, W, H, C, src_stride, 0, views, n_views, dst,
                               dst_stride, interp, flags, slot, 2);
}

int gs360_equirect_views_masked_u8(gs360_ctx* c, const void* const* src_frames, const void* const* mask_frames, int n_frames,
                                   int W, int H, int C, size_t src_stride, size_t mask_stride, const gs360_view* views,
                                   int n_views, void* const* dst, size_t dst_stride, int interp, uint32_t flags, int slot) {
    return equirect_views_impl(c, src_frames, mask_frames, n_frames, W, H, C, src_stride, mask_stride, views, n_views, dst,
                               dst_stride, interp, flags, slot, 1);
}

// ---- host-buffer conveniences ------------------------------------------------------------------
int gs360_equirect_views_u8_host(gs360_ctx* c, const uint8_t* src, int W, int H, int C, size_t src_stride,
                                 const gs360_view* views, int n_views, uint8_t* const* dst, size_t dst_stride,
                                 int interp, uint32_t flags, int slot) {
    return equirect_views_host_impl(c, src, W, H, C, src_stride, views, n_views, (void* const*)dst, dst_stride, interp, flags, slot, 1);
}
int gs360_equirect_views_u16_host(gs360_ctx* c, const uint16_t* src, int W, int H, int C, size_t src_stride,
                                  const gs360_view* views, int n_views, uint16_t* const* dst, size_t dst_stride,
                                  int interp, uint32_t flags, int slot) {
    return equirect_views_host_impl(c, src, W, H, C, src_stride, views, n_views, (void* const*)dst, dst_stride, interp, flags, slot, 2);
}
