// gs360_capi_cloud.hip -- the point-cloud entry points of libgs360hip.so (include/gs360.h): voxel downsampling (VOX-SPEC v1, DESIGN.md
// section 15) and the adaptive octree sampling (OCT-SPEC v1, section 16; gs360_PlyOptimizer.py's adaptive_voxel_downsample,
// PLY:1174-1407).  Validation, the two scratch layouts and the launch sequences of gs360_voxel.hip's and gs360_octree.hip's kernels
// around rocPRIM's stable radix sort (restricted to the keys' significant bits):
//   voxel    keys -> sort -> heads (count, scan, compact) -> pick
//   octree   codes -> sort -> levels -> (host) walk over counts -> ordinals -> sort -> pick -> (host) selection
#include "gs360_capi_internal.h"
#include "gs360_octree.h"
#include "gs360_voxel.h"

#include <chrono>
#include <hipcub/hipcub.hpp>

using namespace gs360;

namespace {

// ---- what both families check and call ---------------------------------------------------------------------------------------------
constexpr size_t kCloudHead = 256;                        // the call's words, in front of either layout

int bit_length(uint64_t v) { return v ? 64 - __builtin_clzll(v) : 0; }

// n_min: a voxel call takes one point, the octree two
int check_n(int64_t n, int64_t n_min) {
    if (n < n_min) return fail(GS360_ERR_ARG, n_min > 1 ? "a cloud of %lld points: the octree takes at least two" : "a cloud of %lld points", (long long)n);
    if (n > GS360_VOXEL_MAX_POINTS) return fail(GS360_ERR_UNSUPPORTED, "a cloud of %lld points: indices are 32-bit, n < 2^31", (long long)n);
    return 0;
}
// a call's cloud and scratch; `rest`: the call's other pointers are all given
int check_cloud(int64_t n, int64_t n_min, const void* xyz_dev, const void* scratch_dev, bool rest = true) {
    if (int rc = check_n(n, n_min)) return rc;
    if (!xyz_dev || !scratch_dev || !rest) return fail(GS360_ERR_ARG, "NULL argument");
    if ((uintptr_t)xyz_dev % 16) return fail(GS360_ERR_ARG, "the cloud is not 16-byte aligned");
    if ((uintptr_t)scratch_dev % 256) return fail(GS360_ERR_ARG, "scratch is not 256-byte aligned");
    return 0;
}
// ... and, once the family's layout is known (the octree checks its own arguments in between), the scratch's size
int check_scratch(size_t scratch_bytes, size_t total, int64_t n) {
    if (scratch_bytes < total) return fail(GS360_ERR_ARG, "scratch of %zu bytes below the %zu a cloud of %lld points needs", scratch_bytes, total, (long long)n);
    return 0;
}

// rocPRIM's stable radix sort of n keys by their bits [0, bits), with their indices (Pairs) or alone; tmp == NULL: the size query
template <bool Pairs, typename K>
hipError_t radix_sort(void* tmp, size_t& bytes, const K* keys_in, K* keys_out, const uint32_t* idx_in, uint32_t* idx_out, int64_t n, int bits,
                      hipStream_t s) {
    if constexpr (Pairs) return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, keys_in, keys_out, idx_in, idx_out, (int)n, 0, bits, s);
    else return hipcub::DeviceRadixSort::SortKeys(tmp, bytes, keys_in, keys_out, (int)n, 0, bits, s);
}
template <typename K>
int sort_query(int64_t n, int bits, size_t* bytes) {
    HIP_TRY((radix_sort<true, K>(nullptr, *bytes, nullptr, nullptr, nullptr, nullptr, n, bits, (hipStream_t)0)));
    return 0;
}
// the sort in the `sort_bytes` carved at `sort`: the size query, its check against the area, the run
template <bool Pairs, typename K>
int stable_sort(void* sort, size_t sort_bytes, const K* keys_in, K* keys_out, const uint32_t* idx_in, uint32_t* idx_out, int64_t n, int bits,
                hipStream_t s) {
    size_t need = 0;
    HIP_TRY(radix_sort<Pairs>(nullptr, need, keys_in, keys_out, idx_in, idx_out, n, bits, s));
    if (need > sort_bytes) return fail(GS360_ERR_INTERNAL, "the sort asks for %zu bytes, the scratch holds %zu", need, sort_bytes);
    need = sort_bytes;
    HIP_TRY(radix_sort<Pairs>(sort, need, keys_in, keys_out, idx_in, idx_out, n, bits, s));
    return 0;
}

// ---- the voxel family ----------------------------------------------------------------------------------------------------------------
struct VoxelArea { size_t partial, keys[2], idx[2], tiles, starts, sort, sort_bytes, total; int64_t n_tiles; };

int voxel_area(int64_t n, VoxelArea* A) {
    size_t sort_bytes = 0;
    if (int rc = sort_query<uint64_t>(n, 64, &sort_bytes)) return rc;
    Carve v;
    v.take(kCloudHead);                                    // error bits, the number of voxels
    A->partial = v.take((size_t)(kVxBoundBlocks + 1) * 8 * sizeof(float), 256);
    for (int b = 0; b < 2; ++b) A->keys[b] = v.take((size_t)n * 8, 256);
    for (int b = 0; b < 2; ++b) A->idx[b] = v.take((size_t)n * 4, 256);
    A->n_tiles = (n + kVxTile - 1) / kVxTile;
    A->tiles = v.take((size_t)A->n_tiles * 4, 256);
    A->starts = v.take((size_t)n * 4, 256);
    A->sort_bytes = round_up(sort_bytes, 256);
    A->sort = v.take(A->sort_bytes, 256);
    A->total = v.at;
    return 0;
}

int check_voxel_call(gs360_ctx* c, const void* xyz_dev, int64_t n, void* scratch_dev, size_t scratch_bytes, int slot, VoxelArea* A) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    if (int rc = check_cloud(n, 1, xyz_dev, scratch_dev)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = voxel_area(n, A)) return rc;
    return check_scratch(scratch_bytes, A->total, n);
}

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

int read_voxel_head(hipStream_t s, const void* scratch_dev, uint32_t* head) {
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
    if (int rc = check_voxel_call(c, xyz_dev, n, scratch_dev, scratch_bytes, slot, &A)) return rc;
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
    HIP_TRY(hipMemsetAsync(base, 0, kCloudHead, s));
    HIP_TRY(launch_voxel_keys(*L, s));
    uint64_t* keys_out = (uint64_t*)(base + A.keys[1]);
    uint32_t* idx_out = (uint32_t*)(base + A.idx[1]);
    const int end_bit = std::max(bits, 1);                // one voxel: a stable sort of one zero bit keeps the order
    if (int rc = with_idx ? stable_sort<true>(base + A.sort, A.sort_bytes, (const uint64_t*)L->keys, keys_out, (const uint32_t*)L->idx, idx_out, n, end_bit, s)
                          : stable_sort<false>(base + A.sort, A.sort_bytes, (const uint64_t*)L->keys, keys_out, nullptr, nullptr, n, end_bit, s))
        return rc;
    L->keys = keys_out;
    if (with_idx) L->idx = idx_out;
    HIP_TRY(launch_voxel_heads(*L, 0, s));
    HIP_TRY(launch_voxel_heads(*L, 1, s));
    uint32_t head[2] = {0, 0};
    if (int rc = read_voxel_head(s, scratch_dev, head)) return rc;
    if (head[1] < 1 || (int64_t)head[1] > n) return fail(GS360_ERR_INTERNAL, "%u voxels of %lld points", head[1], (long long)n);
    *k = head[1];
    return 0;
}

// ---- the octree family ---------------------------------------------------------------------------------------------------------------
// codes[0] holds the ordinals (in, then sorted) once the levels are out; idx[0] the identity permutation once the codes are sorted
struct OctreeArea { size_t codes[2], idx[2], lvl, starts, depth, pick, first, sort, sort_bytes, total; };

int octree_area(int64_t n, OctreeArea* A) {
    size_t wide = 0, narrow = 0;
    if (int rc = sort_query<uint64_t>(n, 3 * kOcDepth, &wide)) return rc;
    if (int rc = sort_query<uint32_t>(n, 32, &narrow)) return rc;
    const size_t words = round_up((size_t)n * 4, 256), leaves = (size_t)n + kOcLeafSlack;
    Carve v;
    v.take(kCloudHead);                                    // the two error words
    for (int b = 0; b < 2; ++b) A->codes[b] = v.take(2 * words, 256);
    for (int b = 0; b < 2; ++b) A->idx[b] = v.take(words, 256);
    A->lvl = v.take((size_t)n, 256);
    A->starts = v.take(leaves * 4, 256);
    A->depth = v.take(leaves, 256);
    A->pick = v.take(leaves * 4, 256);
    A->first = v.take(leaves * 4, 256);
    A->sort_bytes = round_up(std::max(wide, narrow), 256);
    A->sort = v.take(A->sort_bytes, 256);
    A->total = v.at;
    return 0;
}

// the leaves in code order must tile [0, n): nothing else is uploaded
int check_leaves(const std::vector<OcLeaf>& leaves, int64_t n) {
    if (leaves.empty() || leaves.size() >= (size_t)n + kOcLeafSlack) return fail(GS360_ERR_INTERNAL, "%zu leaves of %lld points", leaves.size(), (long long)n);
    uint32_t at = 0;
    for (const OcLeaf& lf : leaves) {
        if (lf.start != at || lf.end <= lf.start || (int64_t)lf.end > n || lf.depth > kOcDepth) return fail(GS360_ERR_INTERNAL, "the leaves do not tile the cloud");
        at = lf.end;
    }
    if ((int64_t)at != n) return fail(GS360_ERR_INTERNAL, "the leaves do not tile the cloud");
    return 0;
}

// the host clock at the end of a stage, after the stream has drained: only when the caller asks for stage times
struct StageClock {
    double* ms; hipStream_t s; std::chrono::steady_clock::time_point t0;
    int mark(int stage) {
        if (!ms) return 0;
        HIP_TRY(hipStreamSynchronize(s));
        const auto t1 = std::chrono::steady_clock::now();
        ms[stage] = std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
        return 0;
    }
};

}  // namespace

int gs360_voxel_scratch(gs360_ctx* c, int64_t n, size_t* bytes) {
    if (!c || !bytes) return fail(GS360_ERR_ARG, "NULL argument");
    if (int rc = check_n(n, 1)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    VoxelArea A;
    if (int rc = voxel_area(n, &A)) return rc;
    *bytes = A.total;
    return GS360_OK;
}

int gs360_cloud_bounds_f32(gs360_ctx* c, const float* xyz_dev, int64_t n, void* scratch_dev, size_t scratch_bytes, float* minmax, int slot) {
    VoxelArea A;
    if (int rc = check_voxel_call(c, xyz_dev, n, scratch_dev, scratch_bytes, slot, &A)) return rc;
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
    return read_voxel_head(s, scratch_dev, head);
}

int gs360_octree_scratch(gs360_ctx* c, int64_t n, size_t* bytes) {
    if (!c || !bytes) return fail(GS360_ERR_ARG, "NULL argument");
    if (int rc = check_n(n, 2)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    OctreeArea A;
    if (int rc = octree_area(n, &A)) return rc;
    *bytes = A.total;
    return GS360_OK;
}

int gs360_octree_pick_f32(gs360_ctx* c, const float* xyz_dev, int64_t n, const float* cube_min, double cube_size, int64_t target,
                          double weight_power, double min_voxel, int strategy, void* scratch_dev, size_t scratch_bytes, uint32_t* pick,
                          uint32_t* order_dev, uint32_t* starts, uint32_t* counts, int64_t* k, double* stage_ms, int slot) {
    if (int rc = check_ctx_slot(c, slot)) return rc;
    if (int rc = check_cloud(n, 2, xyz_dev, scratch_dev, cube_min && k)) return rc;
    if (strategy < GS360_VOXEL_FIRST || strategy > GS360_VOXEL_SEGMENTS) return fail(GS360_ERR_ARG, "unknown strategy %d", strategy);
    if (strategy == GS360_VOXEL_SEGMENTS ? (!order_dev || !starts || !counts) : !pick) return fail(GS360_ERR_ARG, "NULL output");
    if (target < 1 || target >= n) return fail(GS360_ERR_ARG, "a target of %lld for %lld points: 1 <= target < n", (long long)target, (long long)n);
    if (!(cube_size > 0.0) || !std::isfinite(cube_size) || !std::isfinite((float)cube_size)) return fail(GS360_ERR_ARG, "a cube of edge %g", cube_size);
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(cube_min[a])) return fail(GS360_ERR_ARG, "the cube's corner is not finite");
    if (weight_power != weight_power) return fail(GS360_ERR_ARG, "the weight power is not a number");
    if (!std::isfinite(oc_weight(n, weight_power))) return fail(GS360_ERR_UNSUPPORTED, "%lld points to the power %g is no finite weight", (long long)n, weight_power);
    HIP_TRY(hipSetDevice(c->device));
    OctreeArea A;
    if (int rc = octree_area(n, &A)) return rc;
    if (int rc = check_scratch(scratch_bytes, A.total, n)) return rc;

    hipStream_t s = c->stream[slot];
    uint8_t* base = (uint8_t*)scratch_dev;
    const size_t words = round_up((size_t)n * 4, 256);
    OcLaunch L;
    std::memset(&L, 0, sizeof(L));
    L.xyz = xyz_dev; L.n = n;
    for (int a = 0; a < 3; ++a) L.lo[a] = cube_min[a];
    for (int l = 0; l <= kOcDepth; ++l) L.half[l] = (float)(std::ldexp(cube_size, -l) * 0.5);
    L.strategy = strategy == GS360_VOXEL_SEGMENTS ? GS360_VOXEL_FIRST : strategy;
    L.head = (uint32_t*)base;
    L.codes = (uint64_t*)(base + A.codes[0]);
    L.idx = (uint32_t*)(base + A.idx[0]);
    L.lvl = base + A.lvl;
    StageClock clock{stage_ms, s, std::chrono::steady_clock::now()};

    HIP_TRY(hipMemsetAsync(base, 0, kCloudHead, s));
    HIP_TRY(launch_octree_codes(L, s));
    if (int rc = clock.mark(0)) return rc;
    uint64_t* codes_sorted = (uint64_t*)(base + A.codes[1]);
    uint32_t* idx_sorted = (uint32_t*)(base + A.idx[1]);
    if (int rc = stable_sort<true>(base + A.sort, A.sort_bytes, (const uint64_t*)L.codes, codes_sorted, (const uint32_t*)L.idx, idx_sorted, n, 3 * kOcDepth, s)) return rc;
    if (int rc = clock.mark(1)) return rc;
    L.codes = codes_sorted;
    HIP_TRY(launch_octree_levels(L, s));
    if (int rc = clock.mark(2)) return rc;
    std::vector<uint8_t> lvl((size_t)n);
    HIP_TRY(hipMemcpyAsync(lvl.data(), L.lvl, (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (int rc = clock.mark(3)) return rc;

    std::vector<OcLeaf> leaves;
    oc_walk(lvl.data(), n, target, weight_power, min_voxel, cube_size, &leaves);
    std::sort(leaves.begin(), leaves.end(), [](const OcLeaf& a, const OcLeaf& b) { return a.start < b.start; });
    if (int rc = check_leaves(leaves, n)) return rc;
    const size_t m = leaves.size();
    std::vector<uint32_t> h_starts(m), h_out(2 * m);
    std::vector<uint8_t> h_depth(m);
    for (size_t j = 0; j < m; ++j) { h_starts[j] = leaves[j].start; h_depth[j] = leaves[j].depth; }
    if (int rc = clock.mark(4)) return rc;

    L.starts = (const uint32_t*)(base + A.starts); L.depth = base + A.depth; L.n_leaves = (int64_t)m;
    HIP_TRY(hipMemcpyAsync(base + A.starts, h_starts.data(), m * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(base + A.depth, h_depth.data(), m, hipMemcpyHostToDevice, s));
    L.idx = idx_sorted;
    L.ord = (uint32_t*)(base + A.codes[0]);
    L.ident = (uint32_t*)(base + A.idx[0]);
    HIP_TRY(launch_octree_ordinals(L, s));
    if (int rc = clock.mark(5)) return rc;
    uint32_t* ord_sorted = (uint32_t*)(base + A.codes[0] + words);
    if (int rc = stable_sort<true>(base + A.sort, A.sort_bytes, (const uint32_t*)L.ord, ord_sorted, (const uint32_t*)L.ident, idx_sorted, n, std::max(bit_length(m - 1), 1), s)) return rc;
    if (int rc = clock.mark(6)) return rc;
    L.pick = (uint32_t*)(base + A.pick); L.first = (uint32_t*)(base + A.first);
    HIP_TRY(launch_octree_pick(L, s));
    uint32_t head[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(h_out.data(), L.pick, m * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h_out.data() + m, L.first, m * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(head, base, sizeof(head), hipMemcpyDeviceToHost, s));
    if (order_dev) HIP_TRY(hipMemcpyAsync(order_dev, idx_sorted, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (head[0] || head[1]) return fail(GS360_ERR_INTERNAL, head[0] ? "a leaf list left its bound" : "a sorted index left the cloud");
    if (int rc = clock.mark(7)) return rc;

    const std::vector<uint32_t> kept = oc_select(leaves, h_out.data() + m, target, weight_power);
    for (size_t j = 0; j < kept.size(); ++j) {
        if (pick) pick[j] = h_out[kept[j]];
        if (starts) starts[j] = leaves[kept[j]].start;
        if (counts) counts[j] = leaves[kept[j]].end - leaves[kept[j]].start;
    }
    *k = (int64_t)kept.size();
    return clock.mark(8);
}
