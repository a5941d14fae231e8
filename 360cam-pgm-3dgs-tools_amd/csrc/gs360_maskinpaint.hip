// gs360_maskinpaint.hip -- inpainting the masked region of an image (MSK-INPAINT v1).
//
// Reference: gs360_SegmentationMaskTool.py's apply_mode (SEG:809-815), cv2.inpaint(image, mask, 5, INPAINT_TELEA).  Telea's weights
// with a level-ordered march in place of the heap: a pixel of F at distance level k is computed from pixels of lower levels alone,
// so a level's pixels may be computed in any order and one launch per level fills them all.  The steps of a call:
//
//   cols      a lane per column: a sweep down and a sweep up leave every pixel's distance to the nearest pixel outside F in its own
//             column (capped at kMiFar), and count the pixels of F
//   rows      a lane per pixel: the exact squared distance d2 = min over dx of dx^2 + vert(x + dx)^2, searched outward while
//             dx^2 is below the best so far; L = the smallest k with k^2 >= d2, T = sqrtf(d2).  A workgroup counts its levels in LDS
//             and adds the bins it touched to the batch's histogram, and its highest one to the job's K
//   scan      one workgroup: where every level's pixels begin in the list
//   scatter   a lane per pixel: a workgroup reserves, per level it holds, a run of the level's part of the list with one atomic, its
//             lanes take the places of the run.  The order inside a level is whatever the atomics give; no output depends on it
//   fill      a lane per listed pixel of the launch's level: Telea's weighted sum over the offsets (DATA: dy, dx, |r|, 1 / |r|^2)
//             whose pixel lies inside the image at a lower level, three channels in the lane, written in place
//
// No lane waits for another one.  Every loop is bounded (H, kMiFar, the offsets, the jobs); a list entry that is no pixel of the
// launch's level and a pixel without a usable offset set the call's error word.  Floating point is taken op by op (the library is
// built with -ffp-contract=off; no fma here).  The per-lane steps are host-callable (MK_HD) so that
// tests/tools/maskinpaint_hostcheck.hip can step them under a sanitizer.
#include "gs360_maskplane.h"

#pragma clang fp contract(off)

namespace gs360 {
namespace {

MK_HD inline void mi_fail(MiHead* head) { head->err = 1u; }
MK_HD inline bool mi_full(const MiJob& J, const MiHead* head, int j) { return head->filled[j] == (uint32_t)J.H * (uint32_t)J.W; }

// ---- distance --------------------------------------------------------------------------------------------------------------------
// column x: vert = the rows to the nearest pixel outside F above or below, kMiFar from kMiFar on and without one -> the column's pixels of F
MK_HD inline uint32_t mi_cols_lane(const MiJob& J, int x) {
    uint32_t n = 0;
    int run = kMiFar;
    for (int y = 0; y < J.H; ++y) {
        const bool f = J.fill[(int64_t)y * J.fill_stride + x] > 0;
        run = f ? mk_lo(run + 1, kMiFar) : 0;
        n += f;
        J.vert[(int64_t)y * J.W + x] = (uint16_t)run;
    }
    run = kMiFar;
    for (int y = J.H - 1; y >= 0; --y) {
        uint16_t* v = J.vert + (int64_t)y * J.W + x;
        run = *v ? mk_lo(run + 1, kMiFar) : 0;
        if (run < *v) *v = (uint16_t)run;
    }
    return n;
}
// the smallest k with k^2 >= d2, d2 <= kMiMaxLevel^2 (exact in float32): the rounded root is off by one at most
MK_HD inline int mi_level_of(uint32_t d2) {
    int k = (int)sqrtf((float)d2);
    for (int n = 0; n < 2 && (uint32_t)(k * k) < d2; ++n) ++k;
    for (int n = 0; n < 2 && k > 0 && (uint32_t)((k - 1) * (k - 1)) >= d2; ++n) --k;
    return k;
}
// pixel (y, x): stores and returns L, stores T.  A column's candidate is dx^2 + vert^2; one of kMiFar or more is above kMiMaxLevel^2
// whatever its true value, and so is every d2 the search ends on at its bound: such a pixel gets the level kMiFar, which the call
// refuses.  `full`: the job has no pixel outside F and is left alone.
MK_HD inline int mi_rows_lane(const MiJob& J, int y, int x, bool full) {
    const uint16_t* vr = J.vert + (int64_t)y * J.W;
    const int64_t at = (int64_t)y * J.W + x;
    const uint32_t v0 = vr[x];
    if (v0 == 0 || full) {
        J.lev[at] = 0; J.dist[at] = 0.0f;
        return 0;
    }
    uint32_t best = v0 * v0;
    for (int dx = 1; dx < kMiFar && (uint32_t)(dx * dx) < best; ++dx) {
        if (x - dx < 0 && x + dx >= J.W) break;
        if (x - dx >= 0) {
            const uint32_t v = vr[x - dx], c = (uint32_t)(dx * dx) + v * v;
            best = c < best ? c : best;
        }
        if (x + dx < J.W) {
            const uint32_t v = vr[x + dx], c = (uint32_t)(dx * dx) + v * v;
            best = c < best ? c : best;
        }
    }
    const int L = best > (uint32_t)(kMiMaxLevel * kMiMaxLevel) ? kMiFar : mi_level_of(best);
    J.lev[at] = (uint16_t)L; J.dist[at] = sqrtf((float)best);
    return L;
}

// ---- list ------------------------------------------------------------------------------------------------------------------------
// the scan: lane's kMiScanPer levels summed; then, from the sum of the lanes before it, their places
MK_HD inline uint32_t mi_scan_sum(const MiHead* head, int lane) {
    uint32_t n = 0;
    for (int i = lane * kMiScanPer; i < (lane + 1) * kMiScanPer && i <= kMiFar; ++i) n += head->hist[i];
    return n;
}
MK_HD inline void mi_scan_write(MiHead* head, int lane, uint32_t base) {
    for (int i = lane * kMiScanPer; i < (lane + 1) * kMiScanPer && i <= kMiFar; ++i) {
        head->offs[i] = base;
        base += head->hist[i];
    }
}
// the scatter of pixel (y, x): its level if it is listed (else 0) and its rank among the workgroup's pixels of that level ...
MK_HD inline int mi_scatter_rank(const MiJob& J, int y, int x, uint32_t* cnt, uint32_t* rank) {
    const int lv = x < J.W ? J.lev[(int64_t)y * J.W + x] : 0;
    if (lv < 1 || lv > kMiMaxLevel) return 0;
    *rank = mk_atomic_fetch_add(cnt + lv, 1u);
    return lv;
}
// ... and its entry, `run` places into the level's part of the list
MK_HD inline void mi_scatter_put(const MiLaunch& L, const MiJob& J, int y, int x, int lv, uint32_t run) {
    const uint64_t pos = (uint64_t)L.head->offs[lv] + run;
    if (pos < L.list_cap) L.list[pos] = J.px_base + (uint32_t)y * (uint32_t)J.W + (uint32_t)x;
    else mi_fail(L.head);
}

// ---- fill ------------------------------------------------------------------------------------------------------------------------
// (y, x) is inside the image at a level below k
MK_HD inline bool mi_known(const MiJob& J, int y, int x, int k) {
    return y >= 0 && y < J.H && x >= 0 && x < J.W && J.lev[(int64_t)y * J.W + x] < k;
}
// one axis of the image gradient at q from its neighbours before and after (bytes as floats: every difference is exact)
MK_HD inline float mi_grad(float v, float before, float after, bool has_before, bool has_after) {
    if (has_before && has_after) return 0.5f * (after - before);
    if (has_after) return after - v;
    if (has_before) return v - before;
    return 0.0f;
}
// pixel p = (y, x) of level k, in the spec's operation order
MK_HD inline void mi_fill_px(const MiJob& J, int y, int x, int k, MiHead* head) {
    const int W = J.W, H = J.H;
    const float* T = J.dist;
    const float Tp = T[(int64_t)y * W + x];
    const float gx = 0.5f * (T[(int64_t)y * W + mk_lo(x + 1, W - 1)] - T[(int64_t)y * W + mk_hi(x - 1, 0)]);
    const float gy = 0.5f * (T[(int64_t)mk_lo(y + 1, H - 1) * W + x] - T[(int64_t)mk_hi(y - 1, 0) * W + x]);
    float acc[3] = {0.0f, 0.0f, 0.0f}, s = 0.0f;
    for (int i = 0; i < J.n_off && i < kMiMaxOffsets; ++i) {
        const int dy = J.off[2 * i], dx = J.off[2 * i + 1], qy = y + dy, qx = x + dx;
        if (!mi_known(J, qy, qx, k)) continue;
        const float rx = (float)-dx, ry = (float)-dy;
        float dir = fabsf(rx * gx + ry * gy) / J.rlen[i];
        if (dir < 0.01f) dir = 1e-6f;
        const float lev = 1.0f / (1.0f + fabsf(Tp - T[(int64_t)qy * W + qx]));
        const float w = (dir * J.inv2[i]) * lev;
        const bool xb = mi_known(J, qy, qx - 1, k), xa = mi_known(J, qy, qx + 1, k);
        const bool yb = mi_known(J, qy - 1, qx, k), ya = mi_known(J, qy + 1, qx, k);
        const uint8_t* q = J.img + (int64_t)qy * J.img_stride + 3 * (int64_t)qx;
        for (int c = 0; c < 3; ++c) {
            const float v = (float)q[c];
            const float ix = mi_grad(v, xb ? (float)q[c - 3] : 0.0f, xa ? (float)q[c + 3] : 0.0f, xb, xa);
            const float iy = mi_grad(v, yb ? (float)q[c - J.img_stride] : 0.0f, ya ? (float)q[c + J.img_stride] : 0.0f, yb, ya);
            acc[c] = acc[c] + w * ((v + ix * rx) + iy * ry);
        }
        s = s + w;
    }
    if (!(s > 0.0f)) {                                    // MSK-INPAINT's invariant: a pixel of F has a lower level within the radius
        mi_fail(head);
        return;
    }
    uint8_t* p = J.img + (int64_t)y * J.img_stride + 3 * (int64_t)x;
    for (int c = 0; c < 3; ++c) {
        const float o = floorf(acc[c] / s + 0.5f);
        p[c] = (uint8_t)(o < 0.0f ? 0.0f : o > 255.0f ? 255.0f : o);
    }
}
// item i of the launch's level: its list entry -> job and pixel; an entry that is no pixel of that level is a defect and is not filled
MK_HD inline void mi_fill_item(const MiLaunch& L, uint32_t i) {
    const uint64_t pos = (uint64_t)L.head->offs[L.level] + i;
    if (pos >= L.list_cap) return mi_fail(L.head);
    const uint32_t px = L.list[pos];
    int j = 0;
    while (j + 1 < L.n_jobs && j + 1 < GS360_MAX_VIEWS && px >= L.job[j + 1].px_base) ++j;
    const MiJob& J = L.job[j];
    const uint32_t q = px - J.px_base;
    if (q >= (uint32_t)J.H * (uint32_t)J.W || J.lev[q] != L.level) return mi_fail(L.head);
    const int y = (int)(q / (uint32_t)J.W);
    mi_fill_px(J, y, (int)(q - (uint32_t)y * (uint32_t)J.W), L.level, L.head);
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ const MiJob& mi_job(const MiLaunch& L, int* j) {
    *j = job_of(L, blockIdx.x, &MiJob::tile_base);
    return L.job[*j];
}

__global__ void __launch_bounds__(kMiThreads) mi_cols_kernel(const MiLaunch L) {
    int j;
    const MiJob& J = mi_job(L, &j);
    const int64_t x = mk_item_of(J);
    mk_count_tail(x < mi_cols_items(J) ? mi_cols_lane(J, (int)x) : 0u, L.head->filled + j);
}

__global__ void __launch_bounds__(kMiThreads) mi_rows_kernel(const MiLaunch L) {
    __shared__ uint32_t hist[kMiFar + 1];
    int j, y, tx;
    const MiJob& J = mi_job(L, &j);
    mk_tile_of(J, &y, &tx);
    for (int i = threadIdx.x; i <= kMiFar; i += kMiThreads) hist[i] = 0;
    __syncthreads();
    const int x = tx * kMiRowTile.w + threadIdx.x;
    if (x < J.W) {
        const int lv = mi_rows_lane(J, y, x, mi_full(J, L.head, j));
        if (lv) atomicAdd(&hist[lv], 1u);
    }
    __syncthreads();
    uint32_t top = 0;
    for (int i = threadIdx.x; i <= kMiFar; i += kMiThreads)
        if (hist[i]) {
            mk_atomic_add(L.head->hist + i, hist[i]);
            top = (uint32_t)i;
        }
    if (top) mk_atomic_max(L.levels + j, top);
}

__global__ void __launch_bounds__(kMiThreads) mi_scan_kernel(const MiLaunch L) {
    __shared__ uint32_t part[kMiThreads];
    part[threadIdx.x] = mi_scan_sum(L.head, threadIdx.x);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t base = 0;
        for (int i = 0; i < kMiThreads; ++i) {
            const uint32_t n = part[i];
            part[i] = base;
            base += n;
        }
    }
    __syncthreads();
    mi_scan_write(L.head, threadIdx.x, part[threadIdx.x]);
}

__global__ void __launch_bounds__(kMiThreads) mi_scatter_kernel(const MiLaunch L) {
    __shared__ uint32_t cnt[kMiFar + 1], run[kMiFar + 1];
    int j, y, tx;
    const MiJob& J = mi_job(L, &j);
    mk_tile_of(J, &y, &tx);
    for (int i = threadIdx.x; i <= kMiFar; i += kMiThreads) cnt[i] = 0;
    __syncthreads();
    const int x = tx * kMiRowTile.w + threadIdx.x;
    uint32_t rank = 0;
    const int lv = mi_scatter_rank(J, y, x, cnt, &rank);
    __syncthreads();
    for (int i = threadIdx.x; i <= kMiFar; i += kMiThreads)
        if (cnt[i]) run[i] = mk_atomic_fetch_add(L.head->cursor + i, cnt[i]);
    __syncthreads();
    if (lv) mi_scatter_put(L, J, y, x, lv, run[lv] + rank);
}

__global__ void __launch_bounds__(kMiThreads) mi_fill_kernel(const MiLaunch L) {
    const uint32_t i = blockIdx.x * kMiThreads + threadIdx.x;
    if (i < L.items) mi_fill_item(L, i);
}

}  // namespace

hipError_t launch_mask_inpaint(MiStep step, const MiLaunch& L, hipStream_t s) {
    switch (step) {
    case kMiCols: return mk_launch(mi_cols_kernel, L, s);
    case kMiRows: return mk_launch(mi_rows_kernel, L, s);
    case kMiScan: return mk_launch(mi_scan_kernel, L, s);
    case kMiScatter: return mk_launch(mi_scatter_kernel, L, s);
    case kMiFill: return mk_launch(mi_fill_kernel, L, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace gs360
