// gs360_voxel.hip -- voxel downsampling of a resident point cloud (VOX-SPEC v1).
//
// Reference: gs360_PlyOptimizer.py's compute_point_cloud_stats (PLY:110-128), _unique_voxel_count (PLY:846-862) and
// voxel_downsample_by_size (PLY:747-843).  Its np.unique(axis=0) over int64 key triples is a sort of packed keys here: the glue sorts
// (key, index) pairs with rocPRIM's stable radix sort between `keys` and `heads`; this file holds the project's own steps:
//
//   bounds    per-axis float32 minimum and maximum and a count of non-finite coordinates: a grid-stride pass into one record per
//             workgroup, then one workgroup over the records.  No atomics.
//   keys      four points per lane (gs360_cloudsteps.h's pass): k_a = (uint64) floorf((x_a - min_a) / v), one float32 subtract and
//             one correctly rounded float32 divide; packed with x most significant; stored as two 16-byte key stores and one of
//             indices.  A key outside [0, kmax_a] (bounds that do not bound the cloud, a NaN) sets the error word.
//   heads     a sorted key that differs from its predecessor opens a voxel.  Phase 0 counts the heads of every tile of 2048 keys
//             (16-byte loads of two keys per lane, ballots), phase 1 is one workgroup's exclusive scan of the tile counts (the total is
//             the number of voxels), phase 2 ranks the heads of a tile again from ballots and writes the segment starts in key order.
//   pick      a lane owns a voxel: `first` is the segment head; `center` and `centroid` walk the segment in its (ascending original
//             index) order -- the float64 centroid sum point by point, as np.add.at adds -- and keep the first minimum of
//             dist2 = (d0 d0 + d1 d1) + d2 d2.  A segment longer than 32 points is taken over by the lane's whole wavefront.  The
//             pick itself is gs360_cloudsteps.h's, with gs360_voxel.h's target type.
//
// Every loop runs to a bound computed from n (a segment's length, a tile count); a segment list that is not strictly increasing
// inside [0, n) sets the error word instead of being walked.  Floating point is taken op by op (-ffp-contract=off; no fma here).
// The per-lane arithmetic (gs360_voxel.h) is host-callable so that tests/tools/voxel_hostcheck.hip can step it under a sanitizer.
#include "gs360_voxel.h"

#pragma clang fp contract(off)

namespace gs360 {
namespace {

// ---- bounds ----------------------------------------------------------------------------------------------------------------------
struct VxBounds { float mn[3], mx[3], bad; };
__device__ inline void vx_merge(VxBounds& a, const VxBounds& b) {
    for (int c = 0; c < 3; ++c) { a.mn[c] = fminf(a.mn[c], b.mn[c]); a.mx[c] = fmaxf(a.mx[c], b.mx[c]); }
    a.bad = fmaxf(a.bad, b.bad);
}
// a workgroup's lanes' records -> `out` (8 floats), by thread 0
__device__ inline void vx_bounds_store(VxBounds r, float* out) {
    __shared__ VxBounds part[kVxThreads / 64];
    for (int off = 32; off; off >>= 1) {
        VxBounds o;
        for (int c = 0; c < 3; ++c) { o.mn[c] = __shfl_xor(r.mn[c], off); o.mx[c] = __shfl_xor(r.mx[c], off); }
        o.bad = __shfl_xor(r.bad, off);
        vx_merge(r, o);
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kVxThreads / 64; ++w) vx_merge(r, part[w]);
        for (int c = 0; c < 3; ++c) { out[c] = r.mn[c]; out[3 + c] = r.mx[c]; }
        out[6] = r.bad; out[7] = 0.0f;
    }
}
__global__ __launch_bounds__(kVxThreads) void vx_bounds_kernel(VxLaunch L, int phase) {
    VxBounds r;
    for (int c = 0; c < 3; ++c) { r.mn[c] = INFINITY; r.mx[c] = -INFINITY; }
    r.bad = 0.0f;
    if (phase == 0) {
        const int64_t stride = (int64_t)gridDim.x * kVxThreads;
        for (int64_t i = (int64_t)blockIdx.x * kVxThreads + threadIdx.x; i < L.n; i += stride) {
            const float* p = L.xyz + 3 * i;
            for (int c = 0; c < 3; ++c) {
                const float x = p[c];
                if (!isfinite(x)) r.bad = 1.0f;
                r.mn[c] = fminf(r.mn[c], x); r.mx[c] = fmaxf(r.mx[c], x);
            }
        }
        vx_bounds_store(r, L.partial + 8 * (int64_t)blockIdx.x);
    } else {                                               // `phase` records -> the record behind the last workgroup's
        for (int b = threadIdx.x; b < phase; b += kVxThreads) {
            const float* q = L.partial + 8 * (int64_t)b;
            VxBounds o;
            for (int c = 0; c < 3; ++c) { o.mn[c] = q[c]; o.mx[c] = q[3 + c]; }
            o.bad = q[6];
            vx_merge(r, o);
        }
        vx_bounds_store(r, L.partial + 8 * (int64_t)kVxBoundBlocks);
    }
}

// ---- keys ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kVxThreads) void vx_keys_kernel(VxLaunch L) {
    const bool ok = cloud_codes4(L.xyz, L.n, (int64_t)blockIdx.x * kVxThreads + threadIdx.x, L.keys, L.idx,
                                 [&](float x, float y, float z, uint64_t* key) { return vx_point_key(L, x, y, z, key); });
    if (!ok) atomicOr(L.head, kVxErrKey);
}

// ---- heads -----------------------------------------------------------------------------------------------------------------------
// round j of tile t: the lane's two keys from position i on -> whether each opens a voxel
__device__ inline void vx_head_flags(const VxLaunch& L, int64_t i, bool* f0, bool* f1) {
    *f0 = *f1 = false;
    if (i >= L.n) return;
    uint64_t k0, k1 = 0;
    if (i + 1 < L.n) { const ulonglong2 kk = *(const ulonglong2*)(L.keys + i); k0 = kk.x; k1 = kk.y; }   // i is even
    else k0 = L.keys[i];
    *f0 = i == 0 || L.keys[i - 1] != k0;
    *f1 = i + 1 < L.n && k1 != k0;
}
__global__ __launch_bounds__(kVxThreads) void vx_heads_kernel(VxLaunch L, int phase) {
    __shared__ uint32_t wsum[kVxThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t0 = (int64_t)blockIdx.x * kVxTile;
    const uint64_t below = (1ull << lane) - 1;
    uint32_t base = phase ? L.tiles[blockIdx.x] : 0;       // phase 2: the heads in front of this tile; phase 0: this wave's count
    for (int j = 0; j < kVxTile / (2 * kVxThreads); ++j) {
        const int64_t i = t0 + (int64_t)j * 2 * kVxThreads + 2 * threadIdx.x;
        bool f0, f1;
        vx_head_flags(L, i, &f0, &f1);
        const uint64_t b0 = __ballot(f0), b1 = __ballot(f1);
        const uint32_t total = (uint32_t)(__popcll(b0) + __popcll(b1));
        if (!phase) { base += total; continue; }
        if (lane == 0) wsum[wave] = total;
        __syncthreads();
        uint32_t front = 0, all = 0;
        for (int w = 0; w < kVxThreads / 64; ++w) { front += w < wave ? wsum[w] : 0; all += wsum[w]; }
        __syncthreads();
        const uint32_t rank = base + front + (uint32_t)(__popcll(b0 & below) + __popcll(b1 & below));
        if ((f0 || f1) && (int64_t)rank + (f0 && f1) >= L.n) atomicOr(L.head, kVxErrSegment);   // never: there are at most n heads
        else {
            if (f0) L.starts[rank] = (uint32_t)i;
            if (f1) L.starts[rank + f0] = (uint32_t)i + 1;
        }
        base += all;
    }
    if (!phase) {
        if (lane == 0) wsum[wave] = base;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t all = 0;
            for (int w = 0; w < kVxThreads / 64; ++w) all += wsum[w];
            L.tiles[blockIdx.x] = all;
        }
    }
}
// one workgroup: tiles[] -> its exclusive sums, the total into head[1]; a lane owns ceil(n_tiles / 1024) neighbouring tiles
__global__ __launch_bounds__(kVxScanThreads) void vx_scan_kernel(VxLaunch L) {
    __shared__ uint32_t part[kVxScanThreads];
    const int64_t chunk = (L.n_tiles + kVxScanThreads - 1) / kVxScanThreads;
    const int64_t a = threadIdx.x * chunk, b = a + chunk < L.n_tiles ? a + chunk : L.n_tiles;
    uint32_t sum = 0;
    for (int64_t t = a; t < b; ++t) sum += L.tiles[t];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int w = 0; w < kVxScanThreads; ++w) { const uint32_t c = part[w]; part[w] = run; run += c; }
        L.head[1] = run;
    }
    __syncthreads();
    uint32_t run = part[threadIdx.x];
    for (int64_t t = a; t < b; ++t) { const uint32_t c = L.tiles[t]; L.tiles[t] = run; run += c; }
}

// ---- pick ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kVxThreads) void vx_pick_kernel(VxLaunch L, int64_t k) {
    const int64_t g = (int64_t)blockIdx.x * kVxThreads + threadIdx.x;
    int64_t s = 0, e = 0;
    bool valid = g < k;
    if (valid) {
        s = L.starts[g];
        e = g + 1 < k ? (int64_t)L.starts[g + 1] : L.n;
        if (!(s < e && e <= L.n)) { atomicOr(L.head, kVxErrSegment); valid = false; }
    }
    const uint32_t pick = cloud_pick<VxTarget>(L, valid, s, e, valid ? L.keys[s] : 0, threadIdx.x & 63);
    if (valid) L.pick[g] = pick;
}

}  // namespace

hipError_t launch_voxel_bounds(const VxLaunch& L, int phase, hipStream_t s) {
    int64_t blocks = (L.n + 4 * kVxThreads - 1) / (4 * kVxThreads);
    blocks = blocks < 1 ? 1 : blocks > kVxBoundBlocks ? kVxBoundBlocks : blocks;
    if (phase == 0) hipLaunchKernelGGL(vx_bounds_kernel, dim3((unsigned)blocks), dim3(kVxThreads), 0, s, L, 0);
    else hipLaunchKernelGGL(vx_bounds_kernel, dim3(1), dim3(kVxThreads), 0, s, L, (int)blocks);
    return hipGetLastError();
}
hipError_t launch_voxel_keys(const VxLaunch& L, hipStream_t s) {
    const int64_t blocks = (L.n + 4 * kVxThreads - 1) / (4 * kVxThreads);
    hipLaunchKernelGGL(vx_keys_kernel, dim3((unsigned)blocks), dim3(kVxThreads), 0, s, L);
    return hipGetLastError();
}
hipError_t launch_voxel_heads(const VxLaunch& L, int phase, hipStream_t s) {
    if (phase == 1) hipLaunchKernelGGL(vx_scan_kernel, dim3(1), dim3(kVxScanThreads), 0, s, L);
    else hipLaunchKernelGGL(vx_heads_kernel, dim3((unsigned)L.n_tiles), dim3(kVxThreads), 0, s, L, phase);
    return hipGetLastError();
}
hipError_t launch_voxel_pick(const VxLaunch& L, int64_t k, hipStream_t s) {
    const int64_t blocks = (k + kVxThreads - 1) / kVxThreads;
    hipLaunchKernelGGL(vx_pick_kernel, dim3((unsigned)blocks), dim3(kVxThreads), 0, s, L, k);
    return hipGetLastError();
}

}  // namespace gs360
