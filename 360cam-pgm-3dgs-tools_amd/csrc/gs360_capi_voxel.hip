// gs360_capi_voxel.hip -- the point-cloud entry points of libgs360hip.so (include/gs360.h; VOX-SPEC v1):
// validation, the key layout from the cloud's bounds, the scratch layout and the launch sequence of gs360_voxel.hip's kernels around
// rocPRIM's stable radix sort (restricted to the keys' significant bits).
#include "gs360_capi_internal.h"

#include <hipcub/hipcub.hpp>

using namespace gs360;

namespace {

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

constexpr size_t kVxHead = 256;                           // the call's words: error bits, the number of voxels
struct VoxelArea { size_t partial, keys[2], idx[2], tiles, starts, sort, sort_bytes, total; int64_t n_tiles; };

int check_n(int64_t n) {
    if (n < 1) return fail(GS360_ERR_ARG, "a cloud of %lld points", (long long)n);
    if (n > GS360_VOXEL_MAX_POINTS) return fail(GS360_ERR_UNSUPPORTED, "a cloud of %lld points: indices are 32-bit, n < 2^31", (long long)n);
    return 0;
}

int voxel_area(int64_t n, VoxelArea* A) {
    size_t sort_bytes = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr,
                                               (uint32_t*)nullptr, (int)n, 0, 64, (hipStream_t)0));
    size_t at = kVxHead;
    A->partial = at; at += round_up((size_t)(kVxBoundBlocks + 1) * 8 * sizeof(float), 256);
    for (int b = 0; b < 2; ++b) { A->keys[b] = at; at += round_up((size_t)n * 8, 256); }
    for (int b = 0; b < 2; ++b) { A->idx[b] = at; at += round_up((size_t)n * 4, 256); }
    A->n_tiles = (n + kVxTile - 1) / kVxTile;
    A->tiles = at; at += round_up((size_t)A->n_tiles * 4, 256);
    A->starts = at; at += round_up((size_t)n * 4, 256);
    A->sort = at; A->sort_bytes = round_up(sort_bytes, 256); at += A->sort_bytes;
    A->total = at;
    return 0;
}

int check_call(gs360_ctx* c, const void* xyz_dev, int64_t n, void* scratch_dev, size_t scratch_bytes, int slot, VoxelArea* A) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    if (int rc = check_n(n)) return rc;
    if (!xyz_dev || !scratch_dev) return fail(GS360_ERR_ARG, "NULL argument");
    if ((uintptr_t)xyz_dev % 16) return fail(GS360_ERR_ARG, "the cloud is not 16-byte aligned");
    if ((uintptr_t)scratch_dev % 256) return fail(GS360_ERR_ARG, "scratch is not 256-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = voxel_area(n, A)) return rc;
    if (scratch_bytes < A->total) return fail(GS360_ERR_ARG, "scratch of %zu bytes below the %zu a cloud of %lld points needs", scratch_bytes, A->total, (long long)n);
    return 0;
}

int bit_length(uint64_t v) { return v ? 64 - __builtin_clzll(v) : 0; }

// the key layout of a call (VOX-SPEC "Packing"): the largest key per axis from the cloud's maximum by the points' own expression
int key_layout(const float* minmax, double voxel, VxLaunch* L, int* bits) {
    if (!minmax) return fail(GS360_ERR_ARG, "NULL argument");
    if (!(voxel > 0.0)) return fail(GS360_ERR_ARG, "voxel must be > 0");
    const float v = (float)voxel;
    if (!(v > 0.0f) || !std::isfinite(v)) return fail(GS360_ERR_UNSUPPORTED, "a voxel of %g is not a positive float32", voxel);
    int b[3];
    for (int a = 0; a < 3; ++a) {
        const float lo = minmax[a], hi = minmax[3 + a];
        if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo <= hi)) return fail(GS360_ERR_ARG, "the bounds of axis %d are not finite and ordered", a);
        const float q = floorf((hi - lo) / v);
        if (!(q >= 0.0f && q < 9223372036854775808.0f)) return fail(GS360_ERR_UNSUPPORTED, "the keys of axis %d do not fit 63 bits", a);
        L->lo[a] = lo;
        L->kmax[a] = (uint64_t)q;
        b[a] = bit_length(L->kmax[a]);
    }
    *bits = b[0] + b[1] + b[2];
    if (*bits > 64) return fail(GS360_ERR_UNSUPPORTED, "keys of %d + %d + %d bits do not pack into 64", b[0], b[1], b[2]);
    L->v = v;
    L->shift[0] = b[1] + b[2];
    L->shift[1] = b[2];
    return 0;
}

int read_head(hipStream_t s, const void* scratch_dev, uint32_t* head) {
    HIP_TRY(hipMemcpyAsync(head, scratch_dev, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (head[0] & kVxErrKey) return fail(GS360_ERR_ARG, "a point lies outside the bounds given, or is not finite");
    if (head[0]) return fail(GS360_ERR_INTERNAL, "a segment list left its bound");
    return 0;
}

// keys, the sort and the head passes up to the number of voxels; with_idx: (key, index) pairs, for a pick
int sorted_heads(gs360_ctx* c, const float* xyz_dev, int64_t n, const float* minmax, double voxel, void* scratch_dev, size_t scratch_bytes,
                 int slot, bool with_idx, VxLaunch* L, int64_t* k) {
    VoxelArea A;
    if (int rc = check_call(c, xyz_dev, n, scratch_dev, scratch_bytes, slot, &A)) return rc;
    std::memset(L, 0, sizeof(*L));
    int bits = 0;
    if (int rc = key_layout(minmax, voxel, L, &bits)) return rc;
    hipStream_t s = c->stream[slot];
    uint8_t* base = (uint8_t*)scratch_dev;
    L->xyz = xyz_dev; L->n = n;
    L->head = (uint32_t*)base;
    L->keys = (uint64_t*)(base + A.keys[0]);
    L->idx = with_idx ? (uint32_t*)(base + A.idx[0]) : nullptr;
    L->tiles = (uint32_t*)(base + A.tiles); L->n_tiles = A.n_tiles;
    L->starts = (uint32_t*)(base + A.starts);
    HIP_TRY(hipMemsetAsync(base, 0, kVxHead, s));
    HIP_TRY(launch_voxel_keys(*L, s));
    uint64_t* keys_out = (uint64_t*)(base + A.keys[1]);
    uint32_t* idx_out = (uint32_t*)(base + A.idx[1]);
    const int end_bit = std::max(bits, 1);                // one voxel: a stable sort of one zero bit keeps the order
    size_t need = 0;
    if (with_idx) HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, need, (const uint64_t*)L->keys, keys_out, (const uint32_t*)L->idx, idx_out, (int)n, 0, end_bit, s));
    else HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, need, (const uint64_t*)L->keys, keys_out, (int)n, 0, end_bit, s));
    if (need > A.sort_bytes) return fail(GS360_ERR_INTERNAL, "the sort asks for %zu bytes, the scratch holds %zu", need, A.sort_bytes);
    need = A.sort_bytes;
    if (with_idx) HIP_TRY(hipcub::DeviceRadixSort::SortPairs(base + A.sort, need, (const uint64_t*)L->keys, keys_out, (const uint32_t*)L->idx, idx_out, (int)n, 0, end_bit, s));
    else HIP_TRY(hipcub::DeviceRadixSort::SortKeys(base + A.sort, need, (const uint64_t*)L->keys, keys_out, (int)n, 0, end_bit, s));
    L->keys = keys_out;
    if (with_idx) L->idx = idx_out;
    HIP_TRY(launch_voxel_heads(*L, 0, s));
    HIP_TRY(launch_voxel_heads(*L, 1, s));
    uint32_t head[2] = {0, 0};
    if (int rc = read_head(s, scratch_dev, head)) return rc;
    if (head[1] < 1 || (int64_t)head[1] > n) return fail(GS360_ERR_INTERNAL, "%u voxels of %lld points", head[1], (long long)n);
    *k = head[1];
    return 0;
}

}  // namespace

int gs360_voxel_scratch(gs360_ctx* c, int64_t n, size_t* bytes) {
    if (!c || !bytes) return fail(GS360_ERR_ARG, "NULL argument");
    if (int rc = check_n(n)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    VoxelArea A;
    if (int rc = voxel_area(n, &A)) return rc;
    *bytes = A.total;
    return GS360_OK;
}

int gs360_cloud_bounds_f32(gs360_ctx* c, const float* xyz_dev, int64_t n, void* scratch_dev, size_t scratch_bytes, float* minmax, int slot) {
    VoxelArea A;
    if (int rc = check_call(c, xyz_dev, n, scratch_dev, scratch_bytes, slot, &A)) return rc;
    if (!minmax) return fail(GS360_ERR_ARG, "NULL argument");
    hipStream_t s = c->stream[slot];
    VxLaunch L;
    std::memset(&L, 0, sizeof(L));
    L.xyz = xyz_dev; L.n = n;
    L.partial = (float*)((uint8_t*)scratch_dev + A.partial);
    HIP_TRY(launch_voxel_bounds(L, 0, s));
    HIP_TRY(launch_voxel_bounds(L, 1, s));
    float rec[8];
    HIP_TRY(hipMemcpyAsync(rec, L.partial + 8 * (size_t)kVxBoundBlocks, sizeof(rec), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (rec[6] != 0.0f) return fail(GS360_ERR_ARG, "the cloud has non-finite coordinates");
    std::memcpy(minmax, rec, 6 * sizeof(float));
    return GS360_OK;
}

int gs360_voxel_count_f32(gs360_ctx* c, const float* xyz_dev, int64_t n, const float* minmax, double voxel, void* scratch_dev,
                          size_t scratch_bytes, int64_t* count, int slot) {
    if (!count) return fail(GS360_ERR_ARG, "NULL argument");
    VxLaunch L;
    return sorted_heads(c, xyz_dev, n, minmax, voxel, scratch_dev, scratch_bytes, slot, false, &L, count);
}

int gs360_voxel_pick_f32(gs360_ctx* c, const float* xyz_dev, int64_t n, const float* minmax, double voxel, int strategy, void* scratch_dev,
                         size_t scratch_bytes, uint32_t* pick_dev, uint32_t* order_dev, uint32_t* starts_dev, int64_t* k, int slot) {
    if (!k) return fail(GS360_ERR_ARG, "NULL argument");
    if (strategy < GS360_VOXEL_FIRST || strategy > GS360_VOXEL_SEGMENTS) return fail(GS360_ERR_ARG, "unknown strategy %d", strategy);
    if (strategy == GS360_VOXEL_SEGMENTS ? (!order_dev || !starts_dev) : !pick_dev) return fail(GS360_ERR_ARG, "NULL output");
    VxLaunch L;
    if (int rc = sorted_heads(c, xyz_dev, n, minmax, voxel, scratch_dev, scratch_bytes, slot, true, &L, k)) return rc;
    hipStream_t s = c->stream[slot];
    L.strategy = strategy;
    L.pick = pick_dev;
    HIP_TRY(launch_voxel_heads(L, 2, s));
    if (strategy != GS360_VOXEL_SEGMENTS) HIP_TRY(launch_voxel_pick(L, *k, s));
    if (order_dev) HIP_TRY(hipMemcpyAsync(order_dev, L.idx, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    if (starts_dev) HIP_TRY(hipMemcpyAsync(starts_dev, L.starts, (size_t)*k * 4, hipMemcpyDeviceToDevice, s));
    uint32_t head[2] = {0, 0};
    return read_head(s, scratch_dev, head);
}
