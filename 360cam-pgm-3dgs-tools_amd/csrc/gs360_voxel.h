// gs360_voxel.h -- voxel downsampling of a resident point cloud (VOX-SPEC v1): the launch record of
// gs360_voxel.hip's kernels and the per-lane steps that both the device and the host take.  The glue sorts the packed keys between
// `keys` and `heads`; everything else of a count or a pick is one of these steps.  Everything here is host-callable, so that
// tests/tools/voxel_hostcheck.hip can step it under a sanitizer.
#pragma once
#include "gs360_cloudsteps.h"

#pragma clang fp contract(off)

namespace gs360 {

constexpr int kVxThreads = 256;
constexpr int kVxTile = 2048;                            // keys of a workgroup of the head passes: 4 rounds of 2 keys per lane
constexpr int kVxBoundBlocks = 1024;                     // most workgroups (and partial records) of the bounds reduction
constexpr int kVxScanThreads = 1024;                     // the one workgroup that scans the tiles' head counts
constexpr uint32_t kVxErrKey = 1, kVxErrSegment = 2;     // bits of the error word: a key outside the bounds, a broken segment list
struct VxLaunch {
    const float* xyz;                    // n x 3
    int64_t n;
    float lo[3], v;                      // the cloud's minimum, (float) voxel
    uint64_t kmax[3];                    // the largest key per axis (from the cloud's maximum)
    int32_t shift[2];                    // packed = kx << shift[0] | ky << shift[1] | kz
    int32_t strategy, pad;
    float* partial;                      // bounds: kVxBoundBlocks x 8 (min xyz, max xyz, non-finite count, unused)
    uint64_t* keys;                      // n packed keys (built, or sorted)
    uint32_t* idx;                       // n indices (identity when built, the stable order when sorted); NULL: keys alone
    uint32_t* tiles;                     // heads per tile, then their exclusive sums
    int64_t n_tiles;
    uint32_t* starts;                    // k segment starts
    uint32_t* pick;                      // k picks
    uint32_t* head;                      // the call's words: [0] error bits, [1] k
};
hipError_t launch_voxel_bounds(const VxLaunch& L, int phase, hipStream_t s);   // 0: partial records, 1: their reduction into record 0
hipError_t launch_voxel_keys(const VxLaunch& L, hipStream_t s);
hipError_t launch_voxel_heads(const VxLaunch& L, int phase, hipStream_t s);    // 0: count per tile, 1: scan, 2: compact the starts
hipError_t launch_voxel_pick(const VxLaunch& L, int64_t k, hipStream_t s);

CLOUD_HD inline uint64_t vx_mask(int bits) { return bits >= 64 ? ~0ull : (1ull << bits) - 1; }

// one axis' key; false when it lies outside [0, kmax]
CLOUD_HD inline bool vx_axis_key(float x, float lo, float v, uint64_t kmax, uint64_t* k) {
    const float q = floorf((x - lo) / v);
    *k = 0;
    if (!(q >= 0.0f && q < 9223372036854775808.0f)) return false;
    *k = (uint64_t)q;
    return *k <= kmax;
}
CLOUD_HD inline bool vx_point_key(const VxLaunch& L, float x, float y, float z, uint64_t* key) {
    uint64_t kx, ky, kz;
    const bool okx = vx_axis_key(x, L.lo[0], L.v, L.kmax[0], &kx), oky = vx_axis_key(y, L.lo[1], L.v, L.kmax[1], &ky),
               okz = vx_axis_key(z, L.lo[2], L.v, L.kmax[2], &kz), ok = okx && oky && okz;
    *key = (L.shift[0] < 64 ? kx << L.shift[0] : 0) | (ky << L.shift[1]) | kz;
    return ok;
}
// the centre of a packed key's voxel: t_a = min_a + ((float) k_a + 0.5f) * v
CLOUD_HD inline void vx_center(const VxLaunch& L, uint64_t key, float* t) {
    const uint64_t k[3] = {L.shift[0] < 64 ? key >> L.shift[0] : 0, (key >> L.shift[1]) & vx_mask(L.shift[0] - L.shift[1]),
                           key & vx_mask(L.shift[1])};
    for (int a = 0; a < 3; ++a) t[a] = L.lo[a] + ((float)k[a] + 0.5f) * L.v;
}
// the voxel family to gs360_cloudsteps.h: a float64 centroid sum, as np.add.at adds; the centre from the segment's packed key
struct VxTarget {
    using Launch = VxLaunch;
    using Sum = double;
    using Tag = uint64_t;
    CLOUD_HD static void center(const VxLaunch& L, int64_t, uint64_t key, float* t) { vx_center(L, key, t); }
};
// a lane's pick of the segment [s, e) of the sorted indices
CLOUD_HD inline uint32_t vx_pick_lane(const VxLaunch& L, int64_t s, int64_t e, uint64_t key) { return cloud_pick_lane<VxTarget>(L, s, e, key); }

}  // namespace gs360
