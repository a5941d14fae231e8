// gs360_capi_octree.hip -- the adaptive octree sampling's entry points of libgs360hip.so (include/gs360.h; OCT-SPEC v1, DESIGN.md
// section 16; gs360_PlyOptimizer.py's adaptive_voxel_downsample, PLY:1174-1407): validation, the scratch layout and the sequence
// codes -> sort -> levels -> (host) walk over counts -> ordinals -> sort -> pick -> (host) selection around gs360_octree.hip's kernels
// and rocPRIM's stable radix sort.
#include "gs360_capi_internal.h"
#include "gs360_octree.h"

#include <chrono>
#include <hipcub/hipcub.hpp>

using namespace gs360;

namespace {

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

constexpr size_t kOcHead = 256;                           // the call's error words
// codes[0] holds the ordinals (in, then sorted) once the levels are out; idx[0] the identity permutation once the codes are sorted
struct OctreeArea { size_t codes[2], idx[2], lvl, starts, depth, pick, first, sort, sort_bytes, total; };

int check_n(int64_t n) {
    if (n < 2) return fail(GS360_ERR_ARG, "a cloud of %lld points: the octree takes at least two", (long long)n);
    if (n > GS360_VOXEL_MAX_POINTS) return fail(GS360_ERR_UNSUPPORTED, "a cloud of %lld points: indices are 32-bit, n < 2^31", (long long)n);
    return 0;
}

int octree_area(int64_t n, OctreeArea* A) {
    size_t wide = 0, narrow = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, wide, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr,
                                               (uint32_t*)nullptr, (int)n, 0, 3 * kOcDepth, (hipStream_t)0));
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, narrow, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr,
                                               (uint32_t*)nullptr, (int)n, 0, 32, (hipStream_t)0));
    const size_t words = round_up((size_t)n * 4, 256), leaves = (size_t)n + kOcLeafSlack;
    size_t at = kOcHead;
    for (int b = 0; b < 2; ++b) { A->codes[b] = at; at += 2 * words; }
    for (int b = 0; b < 2; ++b) { A->idx[b] = at; at += words; }
    A->lvl = at; at += round_up((size_t)n, 256);
    A->starts = at; at += round_up(leaves * 4, 256);
    A->depth = at; at += round_up(leaves, 256);
    A->pick = at; at += round_up(leaves * 4, 256);
    A->first = at; at += round_up(leaves * 4, 256);
    A->sort = at; A->sort_bytes = round_up(std::max(wide, narrow), 256); at += A->sort_bytes;
    A->total = at;
    return 0;
}

int bit_length(uint64_t v) { return v ? 64 - __builtin_clzll(v) : 0; }

template <typename K>
int sort_pairs(const OctreeArea& A, uint8_t* base, const K* keys_in, K* keys_out, const uint32_t* idx_in, uint32_t* idx_out, int64_t n, int bits,
               hipStream_t s) {
    size_t need = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, need, keys_in, keys_out, idx_in, idx_out, (int)n, 0, bits, s));
    if (need > A.sort_bytes) return fail(GS360_ERR_INTERNAL, "the sort asks for %zu bytes, the scratch holds %zu", need, A.sort_bytes);
    need = A.sort_bytes;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(base + A.sort, need, keys_in, keys_out, idx_in, idx_out, (int)n, 0, bits, s));
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

int gs360_octree_scratch(gs360_ctx* c, int64_t n, size_t* bytes) {
    if (!c || !bytes) return fail(GS360_ERR_ARG, "NULL argument");
    if (int rc = check_n(n)) return rc;
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
    if (int rc = check_n(n)) return rc;
    if (!xyz_dev || !scratch_dev || !cube_min || !k) return fail(GS360_ERR_ARG, "NULL argument");
    if ((uintptr_t)xyz_dev % 16) return fail(GS360_ERR_ARG, "the cloud is not 16-byte aligned");
    if ((uintptr_t)scratch_dev % 256) return fail(GS360_ERR_ARG, "scratch is not 256-byte aligned");
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
    if (scratch_bytes < A.total) return fail(GS360_ERR_ARG, "scratch of %zu bytes below the %zu a cloud of %lld points needs", scratch_bytes, A.total, (long long)n);

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

    HIP_TRY(hipMemsetAsync(base, 0, kOcHead, s));
    HIP_TRY(launch_octree_codes(L, s));
    if (int rc = clock.mark(0)) return rc;
    uint64_t* codes_sorted = (uint64_t*)(base + A.codes[1]);
    uint32_t* idx_sorted = (uint32_t*)(base + A.idx[1]);
    if (int rc = sort_pairs(A, base, (const uint64_t*)L.codes, codes_sorted, (const uint32_t*)L.idx, idx_sorted, n, 3 * kOcDepth, s)) return rc;
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
    if (int rc = sort_pairs(A, base, (const uint32_t*)L.ord, ord_sorted, (const uint32_t*)L.ident, idx_sorted, n, std::max(bit_length(m - 1), 1), s)) return rc;
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
