// gs360_cloudsteps.h -- the steps the two point-cloud families share (gs360_voxel.hip, VOX-SPEC v1, DESIGN.md section 15;
// gs360_octree.hip, OCT-SPEC v1, section 16): the squared distance, the pick of a segment of an index array by its lane or, when it
// is longer than kCloudLaneMax points, by the lane's wavefront, and the four-points-per-lane pass that writes a code per point.
// A family names itself by a target type T:
//   T::Launch   its launch record, with `xyz` (n x 3), `idx` (the indices the segments are cut from) and `strategy`
//   T::Sum      the centroid's accumulator: double for a voxel (np.add.at on float64), float for a leaf (pts.mean on float32)
//   T::Tag      what travels with a segment to its centre: a voxel's packed key, a leaf's depth
//   T::center   the centre of the segment that starts at s
// What differs (the per-point codes, the head and scan passes, the levels and ordinals, the error words) stays in the families'
// files.  Floating point is taken op by op.  The per-lane steps are host-callable, so that tests/tools/voxel_hostcheck.hip and
// tests/tools/octree_hostcheck.hip can step them under a sanitizer.
#pragma once
#include "gs360_kernels.h"

#pragma clang fp contract(off)

namespace gs360 {

#define CLOUD_HD __host__ __device__

constexpr int kCloudLaneMax = 32;                        // a longer segment is picked by its wavefront, not by its lane
constexpr uint32_t kCloudNone = 0xFFFFFFFFu;             // a position in a segment: none yet

CLOUD_HD inline float cloud_dist2(const float* p, const float* t) {
    const float d0 = p[0] - t[0], d1 = p[1] - t[1], d2 = p[2] - t[2];
    return (d0 * d0 + d1 * d1) + d2 * d2;
}

// a lane's pick of the segment [s, e) of L.idx: `first` is the segment head; `center` and `centroid` walk the segment in its order
// -- the centroid sum point by point -- and keep the first minimum of the squared distance
template <class T>
CLOUD_HD inline uint32_t cloud_pick_lane(const typename T::Launch& L, int64_t s, int64_t e, typename T::Tag tag) {
    using Sum = typename T::Sum;
    const uint32_t head = L.idx[s];
    if (L.strategy == GS360_VOXEL_FIRST || e - s == 1) return head;   // a single point is its own centroid and the only candidate
    float t[3];
    if (L.strategy == GS360_VOXEL_CENTER) T::center(L, s, tag, t);
    else {
        Sum sum[3] = {0, 0, 0};
        for (int64_t p = s; p < e; ++p) {
            const float* q = L.xyz + 3 * (int64_t)L.idx[p];
            sum[0] += (Sum)q[0]; sum[1] += (Sum)q[1]; sum[2] += (Sum)q[2];
        }
        const Sum cnt = (Sum)(e - s);
        for (int a = 0; a < 3; ++a) t[a] = (float)(sum[a] / cnt);
    }
    uint32_t best_i = head;
    float best = cloud_dist2(L.xyz + 3 * (int64_t)best_i, t);
    for (int64_t p = s + 1; p < e; ++p) {
        const uint32_t i = L.idx[p];
        const float d = cloud_dist2(L.xyz + 3 * (int64_t)i, t);
        if (d < best) { best = d; best_i = i; }
    }
    return best_i;
}

// the wavefront's pick of the long segment [s, e): 64 points are fetched at a time, the centroid sum still runs over them one by
// one (every lane adds the same shuffled values in the same order), and the minimum is reduced as (dist2, position) pairs, so ties
// still go to the earliest point.  Every lane returns the same index.
template <class T>
__device__ inline uint32_t cloud_pick_wave(const typename T::Launch& L, int64_t s, int64_t e, typename T::Tag tag, int lane) {
    using Sum = typename T::Sum;
    float t[3];
    if (L.strategy == GS360_VOXEL_CENTER) T::center(L, s, tag, t);
    else {
        Sum sum[3] = {0, 0, 0};
        for (int64_t base = s; base < e; base += 64) {
            float p[3] = {0.0f, 0.0f, 0.0f};
            if (base + lane < e) {
                const float* q = L.xyz + 3 * (int64_t)L.idx[base + lane];
                p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
            }
            const int cnt = e - base < 64 ? (int)(e - base) : 64;
            for (int j = 0; j < cnt; ++j) {                // in segment order, in every lane alike
                sum[0] += (Sum)__shfl(p[0], j); sum[1] += (Sum)__shfl(p[1], j); sum[2] += (Sum)__shfl(p[2], j);
            }
        }
        const Sum cnt = (Sum)(e - s);
        for (int a = 0; a < 3; ++a) t[a] = (float)(sum[a] / cnt);
    }
    float best = INFINITY;
    uint32_t at = kCloudNone;                              // position in the segment
    for (int64_t base = s; base < e; base += 64) {
        if (base + lane < e) {
            const float d = cloud_dist2(L.xyz + 3 * (int64_t)L.idx[base + lane], t);
            if (at == kCloudNone || d < best) { best = d; at = (uint32_t)(base + lane - s); }
        }
    }
    for (int off = 32; off; off >>= 1) {
        const float ob = __shfl_xor(best, off);
        const uint32_t oa = __shfl_xor(at, off);
        if (oa != kCloudNone && (at == kCloudNone || ob < best || (ob == best && oa < at))) { best = ob; at = oa; }
    }
    return L.idx[s + at];
}

// a lane's segment [s, e) (`valid`: it has one) -> its pick.  A short segment is the lane's own; the long ones of a wavefront are
// balloted and walked one after another by the whole wavefront, each result given back to its lane.  Called by whole wavefronts.
template <class T>
__device__ inline uint32_t cloud_pick(const typename T::Launch& L, bool valid, int64_t s, int64_t e, typename T::Tag tag, int lane) {
    const bool wide = valid && e - s > kCloudLaneMax && L.strategy != GS360_VOXEL_FIRST;
    uint32_t pick = 0;
    if (valid && !wide) pick = cloud_pick_lane<T>(L, s, e, tag);
    uint64_t todo = __ballot(wide);                        // the same in every lane: the wavefront stays whole below
    while (todo) {
        const int l = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int64_t ws = __shfl(s, l), we = __shfl(e, l);
        const uint32_t got = cloud_pick_wave<T>(L, ws, we, __shfl(tag, l), lane);
        if (lane == l) pick = got;
    }
    return pick;
}

// lane g's four points of the cloud (three 16-byte loads: the cloud is 16-byte aligned) -> their codes by `code(x, y, z, &c)` as two
// 16-byte stores and, where `idx` is given, their own indices as one; the last one to three points go one by one.  -> whether
// every call of `code` returned true
template <class F>
__device__ inline bool cloud_codes4(const float* xyz, int64_t n, int64_t g, uint64_t* codes, uint32_t* idx, F code) {
    const int64_t p0 = 4 * g;
    if (p0 >= n) return true;
    uint64_t c[4];
    bool ok = true;
    if (p0 + 4 <= n) {
        const float4* src = (const float4*)xyz + 3 * g;         // 48 bytes per lane
        const float4 u = src[0], v = src[1], w = src[2];
        ok &= code(u.x, u.y, u.z, &c[0]);
        ok &= code(u.w, v.x, v.y, &c[1]);
        ok &= code(v.z, v.w, w.x, &c[2]);
        ok &= code(w.y, w.z, w.w, &c[3]);
        ((ulonglong2*)(codes + p0))[0] = make_ulonglong2(c[0], c[1]);
        ((ulonglong2*)(codes + p0))[1] = make_ulonglong2(c[2], c[3]);
        if (idx) *(uint4*)(idx + p0) = make_uint4((uint32_t)p0, (uint32_t)p0 + 1, (uint32_t)p0 + 2, (uint32_t)p0 + 3);
    } else {
        for (int64_t p = p0; p < n; ++p) {
            const float* q = xyz + 3 * p;
            ok &= code(q[0], q[1], q[2], &c[0]);
            codes[p] = c[0];
            if (idx) idx[p] = (uint32_t)p;
        }
    }
    return ok;
}

}  // namespace gs360
