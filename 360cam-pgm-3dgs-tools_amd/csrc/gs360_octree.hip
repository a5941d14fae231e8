// gs360_octree.hip -- the kernels of the adaptive octree sampling (OCT-SPEC v1; gs360_PlyOptimizer.py's
// adaptive_voxel_downsample, PLY:1174-1407).  The glue sorts (code, index) pairs after `codes` and (ordinal, index) pairs after
// `ordinals` with rocPRIM's stable radix sort, and walks the tree over counts on the host between `levels` and `ordinals`; the
// per-point, per-pair and per-leaf arithmetic is gs360_octree.h's, the four-point pass and the pick gs360_cloudsteps.h's.
//
//   codes     four points per lane (three 16-byte loads): the 36-bit path code by the float32 add chain; two 16-byte code stores and
//             one of indices.
//   levels    four sorted positions per lane: the level at which each code leaves its predecessor's, as one 4-byte store.
//   ordinals  a lane per sorted position: the leaf that holds it, by bisection of the leaf starts (32 rounds at the most), written at
//             the point's original index; and the identity permutation that the second sort orders.
//   pick      a lane owns a leaf and walks its points in ascending original index.  A leaf longer than 32 points is taken over by
//             the lane's whole wavefront (gs360_cloudsteps.h, with gs360_octree.h's target type: a float32 centroid sum).
//
// Every loop runs to a bound computed from n or a leaf's length; a leaf list that is not strictly increasing inside [0, n), or a
// sorted index outside it, sets the error word instead of being followed.
#include "gs360_octree.h"

namespace gs360 {
namespace {

__global__ __launch_bounds__(kOcThreads) void oc_codes_kernel(OcLaunch L) {
    cloud_codes4(L.xyz, L.n, (int64_t)blockIdx.x * kOcThreads + threadIdx.x, L.codes, L.idx, [&](float x, float y, float z, uint64_t* code) {
        *code = oc_point_code(L, x, y, z);
        return true;                                       // every point has a path
    });
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

__global__ __launch_bounds__(kOcThreads) void oc_pick_kernel(OcLaunch L) {
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
    const uint32_t pick = cloud_pick<OcTarget>(L, valid, s, e, depth, threadIdx.x & 63);
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
