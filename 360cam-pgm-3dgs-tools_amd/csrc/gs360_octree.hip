// gs360_octree.hip -- the kernels of the adaptive octree sampling (OCT-SPEC v1; gs360_PlyOptimizer.py's
// adaptive_voxel_downsample, PLY:1174-1407).  The glue sorts (code, index) pairs after `codes` and (ordinal, index) pairs after
// `ordinals` with rocPRIM's stable radix sort, and walks the tree over counts on the host between `levels` and `ordinals`; the
// per-point, per-pair and per-leaf arithmetic is gs360_octree.h's.
//
//   codes     four points per lane (three 16-byte loads): the 36-bit path code by the float32 add chain; two 16-byte code stores and
//             one of indices.
//   levels    four sorted positions per lane: the level at which each code leaves its predecessor's, as one 4-byte store.
//   ordinals  a lane per sorted position: the leaf that holds it, by bisection of the leaf starts (32 rounds at the most), written at
//             the point's original index; and the identity permutation that the second sort orders.
//   pick      a lane owns a leaf and walks its points in ascending original index.  A leaf longer than 32 points is taken over by
//             the lane's whole wavefront: 64 points are fetched at a time, the float32 sum still runs over them one by one (every lane
//             adds the same shuffled values in the same order), the minimum is reduced as (dist2, position) pairs.
//
// Every loop runs to a bound computed from n or a leaf's length; a leaf list that is not strictly increasing inside [0, n), or a
// sorted index outside it, sets the error word instead of being followed.
#include "gs360_octree.h"

namespace gs360 {
namespace {

__global__ __launch_bounds__(kOcThreads) void oc_codes_kernel(OcLaunch L) {
    const int64_t g = (int64_t)blockIdx.x * kOcThreads + threadIdx.x, p0 = 4 * g;
    if (p0 >= L.n) return;
    if (p0 + 4 <= L.n) {
        const float4* src = (const float4*)L.xyz + 3 * g;       // 48 bytes per lane: the cloud is 16-byte aligned
        const float4 a = src[0], b = src[1], c = src[2];
        const uint64_t c0 = oc_point_code(L, a.x, a.y, a.z), c1 = oc_point_code(L, a.w, b.x, b.y), c2 = oc_point_code(L, b.z, b.w, c.x),
                       c3 = oc_point_code(L, c.y, c.z, c.w);
        ((ulonglong2*)(L.codes + p0))[0] = make_ulonglong2(c0, c1);
        ((ulonglong2*)(L.codes + p0))[1] = make_ulonglong2(c2, c3);
        *(uint4*)(L.idx + p0) = make_uint4((uint32_t)p0, (uint32_t)p0 + 1, (uint32_t)p0 + 2, (uint32_t)p0 + 3);
    } else {
        for (int64_t p = p0; p < L.n; ++p) {
            const float* q = L.xyz + 3 * p;
            L.codes[p] = oc_point_code(L, q[0], q[1], q[2]);
            L.idx[p] = (uint32_t)p;
        }
    }
}

__global__ __launch_bounds__(kOcThreads) void oc_levels_kernel(OcLaunch L) {
    const int64_t g = (int64_t)blockIdx.x * kOcThreads + threadIdx.x, p0 = 4 * g;
    if (p0 >= L.n) return;
    const uint64_t prev = p0 ? L.codes[p0 - 1] : 0;
    if (p0 + 4 <= L.n) {
        const ulonglong2 a = ((const ulonglong2*)(L.codes + p0))[0], b = ((const ulonglong2*)(L.codes + p0))[1];
        const uint32_t l0 = p0 ? oc_level(prev, a.x) : 0, l1 = oc_level(a.x, a.y), l2 = oc_level(a.y, b.x), l3 = oc_level(b.x, b.y);
        *(uint32_t*)(L.lvl + p0) = l0 | l1 << 8 | l2 << 16 | l3 << 24;
    } else {
        uint64_t before = prev;
        for (int64_t p = p0; p < L.n; ++p) {
            const uint64_t cur = L.codes[p];
            L.lvl[p] = p ? oc_level(before, cur) : 0;
            before = cur;
        }
    }
}

__global__ __launch_bounds__(kOcThreads) void oc_ordinals_kernel(OcLaunch L) {
    const int64_t p = (int64_t)blockIdx.x * kOcThreads + threadIdx.x;
    if (p >= L.n) return;
    int64_t lo = 0, hi = L.n_leaves;                       // starts[lo] <= p < starts[hi] (starts[0] = 0, starts[n_leaves] = n)
    for (int it = 0; it < 32; ++it) {
        if (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)L.starts[mid] <= p) lo = mid; else hi = mid;
        }
    }
    const uint32_t i = L.idx[p];
    if (i < L.n) L.ord[i] = (uint32_t)lo;
    else L.head[1] = kOcErrIndex;                          // never: the sort permutes [0, n)
    L.ident[p] = (uint32_t)p;
}

// the wavefront's pick of the long leaf [s, e): every lane returns the same index
__device__ inline uint32_t oc_pick_wave(const OcLaunch& L, int64_t s, int64_t e, int depth, int lane) {
    float t[3];
    if (L.strategy == GS360_VOXEL_CENTER) oc_center(L, L.idx[s], depth, t);
    else {
        float sum[3] = {0.0f, 0.0f, 0.0f};
        for (int64_t base = s; base < e; base += 64) {
            float p[3] = {0.0f, 0.0f, 0.0f};
            if (base + lane < e) {
                const float* q = L.xyz + 3 * (int64_t)L.idx[base + lane];
                p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
            }
            const int cnt = e - base < 64 ? (int)(e - base) : 64;
            for (int j = 0; j < cnt; ++j) {                // in index order, in every lane alike
                sum[0] += __shfl(p[0], j); sum[1] += __shfl(p[1], j); sum[2] += __shfl(p[2], j);
            }
        }
        const float cnt = (float)(e - s);
        for (int a = 0; a < 3; ++a) t[a] = sum[a] / cnt;
    }
    float best = INFINITY;
    uint32_t at = 0xFFFFFFFFu;                             // position in the leaf; none yet
    for (int64_t base = s; base < e; base += 64) {
        if (base + lane < e) {
            const float d = oc_dist2(L.xyz + 3 * (int64_t)L.idx[base + lane], t);
            if (at == 0xFFFFFFFFu || d < best) { best = d; at = (uint32_t)(base + lane - s); }
        }
    }
    for (int off = 32; off; off >>= 1) {
        const float ob = __shfl_xor(best, off);
        const uint32_t oa = __shfl_xor(at, off);
        if (oa != 0xFFFFFFFFu && (at == 0xFFFFFFFFu || ob < best || (ob == best && oa < at))) { best = ob; at = oa; }
    }
    return L.idx[s + at];
}
__global__ __launch_bounds__(kOcThreads) void oc_pick_kernel(OcLaunch L) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * kOcThreads + threadIdx.x;
    int64_t s = 0, e = 0;
    int depth = 0;
    bool valid = g < L.n_leaves;
    if (valid) {
        s = L.starts[g];
        e = g + 1 < L.n_leaves ? (int64_t)L.starts[g + 1] : L.n;
        depth = L.depth[g];
        if (!(s < e && e <= L.n && depth <= kOcDepth)) { L.head[0] = kOcErrLeaf; valid = false; }
    }
    const bool wide = valid && e - s > kOcLaneMax && L.strategy != GS360_VOXEL_FIRST;
    uint32_t pick = 0;
    if (valid && !wide) pick = oc_pick_lane(L, s, e, depth);
    uint64_t todo = __ballot(wide);                        // the same in every lane: the wavefront stays whole below
    while (todo) {
        const int l = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int64_t ws = __shfl(s, l), we = __shfl(e, l);
        const uint32_t got = oc_pick_wave(L, ws, we, __shfl(depth, l), lane);
        if (lane == l) pick = got;
    }
    if (valid) { L.pick[g] = pick; L.first[g] = L.idx[s]; }
}

}  // namespace

hipError_t launch_octree_codes(const OcLaunch& L, hipStream_t s) {
    const int64_t blocks = (L.n + 4 * kOcThreads - 1) / (4 * kOcThreads);
    hipLaunchKernelGGL(oc_codes_kernel, dim3((unsigned)blocks), dim3(kOcThreads), 0, s, L);
    return hipGetLastError();
}
hipError_t launch_octree_levels(const OcLaunch& L, hipStream_t s) {
    const int64_t blocks = (L.n + 4 * kOcThreads - 1) / (4 * kOcThreads);
    hipLaunchKernelGGL(oc_levels_kernel, dim3((unsigned)blocks), dim3(kOcThreads), 0, s, L);
    return hipGetLastError();
}
hipError_t launch_octree_ordinals(const OcLaunch& L, hipStream_t s) {
    const int64_t blocks = (L.n + kOcThreads - 1) / kOcThreads;
    hipLaunchKernelGGL(oc_ordinals_kernel, dim3((unsigned)blocks), dim3(kOcThreads), 0, s, L);
    return hipGetLastError();
}
hipError_t launch_octree_pick(const OcLaunch& L, hipStream_t s) {
    const int64_t blocks = (L.n_leaves + kOcThreads - 1) / kOcThreads;
    hipLaunchKernelGGL(oc_pick_kernel, dim3((unsigned)blocks), dim3(kOcThreads), 0, s, L);
    return hipGetLastError();
}

}  // namespace gs360
