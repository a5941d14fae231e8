// gs360_octree.h -- adaptive octree sampling of a resident point cloud (OCT-SPEC v1): the launch record of
// gs360_octree.hip's kernels and the steps that both the device and the host take.
//
// Reference: gs360_PlyOptimizer.py's adaptive_voxel_downsample (PLY:1174-1407).  Its tree of index arrays is one stable sort of
// 36-bit path codes here: a node is a range of the sorted array, its children are the sub-ranges cut where the code first differs
// at the next level.  The split order is a serial priority queue, but it looks at counts only (oc_walk, host); what touches points
// is per point (oc_descend: the octant at every level by the reference's own float32 add chain), per sorted pair (oc_level) or per
// leaf (oc_pick_lane, gs360_cloudsteps.h's pick with OcTarget: over the leaf's points in ascending original index, the float32
// centroid sum point by point as pts.mean(axis=0) adds).  Floating point is taken op by op.  Everything here is host-callable, so that
// tests/tools/octree_hostcheck.hip can step it under a sanitizer.
#pragma once
#include <algorithm>
#include <cmath>
#include <queue>
#include <vector>

#include "gs360_cloudsteps.h"

#pragma clang fp contract(off)

namespace gs360 {

constexpr int kOcDepth = 12;                             // the reference's max_depth; 3 bits per level: codes of 36 bits
constexpr int kOcThreads = 256;
constexpr int kOcLeafSlack = 8;                          // a split adds at most 7 to leaves + heap: there are fewer than n + 8 leaves
constexpr uint32_t kOcErrLeaf = 1, kOcErrIndex = 2;      // error words (plain stores, a word each): a broken leaf list, an index outside [0, n)
constexpr double kOcEps = 1e-9;

struct OcLaunch {
    const float* xyz;                    // n x 3
    int64_t n;
    float lo[3];                         // the cube's minimum corner
    float half[kOcDepth + 1];            // (float) (size_l * 0.5), size_l = cube_size * 0.5^l: the add chain's step at level l
    int32_t strategy;                    // GS360_VOXEL_FIRST / _CENTER / _CENTROID
    uint64_t* codes;                     // n path codes (built, or sorted)
    uint32_t* idx;                       // n indices: identity when built, in code order after the first sort, grouped by leaf (ascending
                                         // inside a leaf) after the second
    uint8_t* lvl;                        // per sorted position: the first level at which its code leaves its predecessor's (13: equal)
    const uint32_t* starts;              // n_leaves leaf starts in code order; leaf j ends where leaf j + 1 starts (the last at n)
    const uint8_t* depth;                // n_leaves depths
    int64_t n_leaves;
    uint32_t* ord;                       // per original point: its leaf's ordinal
    uint32_t* ident;                     // the identity permutation the second sort orders
    uint32_t* pick;                      // n_leaves representatives
    uint32_t* first;                     // n_leaves smallest indices
    uint32_t* head;                      // the call's words: [0] kOcErrLeaf or 0, [1] kOcErrIndex or 0
};
hipError_t launch_octree_codes(const OcLaunch& L, hipStream_t s);
hipError_t launch_octree_levels(const OcLaunch& L, hipStream_t s);
hipError_t launch_octree_ordinals(const OcLaunch& L, hipStream_t s);
hipError_t launch_octree_pick(const OcLaunch& L, hipStream_t s);

// the add chain over the first `levels` (<= 12) levels of p's path: m = the corner reached, *next = the step of the level after
// them (the half of that node); returns the child codes passed, the top level most significant
CLOUD_HD inline uint64_t oc_descend(const OcLaunch& L, const float* p, int levels, float* m, float* next) {
    uint64_t code = 0;
    float h = L.half[0];
    for (int a = 0; a < 3; ++a) m[a] = L.lo[a];
#pragma unroll
    for (int l = 0; l < kOcDepth; ++l) {
        if (l < levels) {
            uint32_t child = 0;
            for (int a = 0; a < 3; ++a) {
                const float c = m[a] + h;
                const bool bit = p[a] >= c;
                m[a] = bit ? c : m[a];
                child = child << 1 | (uint32_t)bit;
            }
            code = code << 3 | child;
            h = L.half[l + 1];
        }
    }
    *next = h;
    return code;
}
CLOUD_HD inline uint64_t oc_point_code(const OcLaunch& L, float x, float y, float z) {
    const float p[3] = {x, y, z};
    float m[3], next;
    return oc_descend(L, p, kOcDepth, m, &next);
}
// the first level (1..12) at which two codes differ; 13 when they are equal
CLOUD_HD inline uint8_t oc_level(uint64_t prev, uint64_t cur) {
    const uint64_t x = (prev ^ cur) & ((1ull << (3 * kOcDepth)) - 1);
    if (!x) return kOcDepth + 1;
    return (uint8_t)(kOcDepth - (63 - __builtin_clzll(x)) / 3);
}
// the centre of the leaf of depth `depth` that holds point i
CLOUD_HD inline void oc_center(const OcLaunch& L, uint32_t i, int depth, float* t) {
    float h;
    oc_descend(L, L.xyz + 3 * (int64_t)i, depth, t, &h);
    for (int a = 0; a < 3; ++a) t[a] = t[a] + h;
}
// the octree family to gs360_cloudsteps.h: a float32 centroid sum, as pts.mean(axis=0) adds; the centre from the head point's add
// chain to the leaf's depth
struct OcTarget {
    using Launch = OcLaunch;
    using Sum = float;
    using Tag = int;
    CLOUD_HD static void center(const OcLaunch& L, int64_t s, int depth, float* t) { oc_center(L, L.idx[s], depth, t); }
};
// a lane's pick of the leaf [s, e) of the indices grouped by leaf
CLOUD_HD inline uint32_t oc_pick_lane(const OcLaunch& L, int64_t s, int64_t e, int depth) { return cloud_pick_lane<OcTarget>(L, s, e, depth); }

// ---- the serial part: counts only (host) -------------------------------------------------------------------------------------------
struct OcLeaf { uint32_t start, end; uint8_t depth; };

// Python's float(count) ** power; a negative power counts as 0 (PLY:1244-1254)
inline double oc_weight(int64_t count, double power) { return power > 0.0 ? std::pow((double)count, power) : 1.0; }

// the split loop (PLY:1275-1348) over ranges of the sorted array: lvl[n] as oc_level writes it (lvl[0] is not read); a node's
// children are cut where lvl == depth + 1.  min_voxel == 0: none.  Leaves come out in the order the loop made them.
inline void oc_walk(const uint8_t* lvl, int64_t n, int64_t target, double power, double min_voxel, double cube_size, std::vector<OcLeaf>* leaves) {
    struct Node { double negw; int64_t seq; uint32_t start, end; uint8_t depth; };
    struct Later { bool operator()(const Node& a, const Node& b) const { return a.negw > b.negw || (a.negw == b.negw && a.seq > b.seq); } };
    std::priority_queue<Node, std::vector<Node>, Later> heap;
    int64_t seq = 0;
    leaves->clear();
    heap.push({-oc_weight(n, power), seq++, 0u, (uint32_t)n, 0});
    while (!heap.empty() && (int64_t)(leaves->size() + heap.size()) < target) {
        const Node node = heap.top();
        heap.pop();
        const double size = std::ldexp(cube_size, -(int)node.depth);
        if (node.end - node.start <= 1 || node.depth >= kOcDepth || (min_voxel != 0.0 && size <= min_voxel + kOcEps) || size * 0.5 <= kOcEps) {
            leaves->push_back({node.start, node.end, node.depth});
            continue;
        }
        const uint8_t d = node.depth + 1;
        uint32_t a = node.start;
        for (uint32_t p = node.start + 1; p <= node.end; ++p) {
            if (p < node.end && lvl[p] > d) continue;
            if (p - a == 1) leaves->push_back({a, p, d});
            else heap.push({-oc_weight(p - a, power), seq++, a, p, d});
            a = p;
        }
        if ((int64_t)(leaves->size() + heap.size()) >= target) break;
    }
    for (; !heap.empty(); heap.pop()) leaves->push_back({heap.top().start, heap.top().end, heap.top().depth});
}

// the leaves kept, in output order (PLY:1358-1363): weight and count descending, then the smallest original index ascending;
// first[j] = that index of leaf j.  -> positions into `leaves`
inline std::vector<uint32_t> oc_select(const std::vector<OcLeaf>& leaves, const uint32_t* first, int64_t target, double power) {
    std::vector<uint32_t> at(leaves.size());
    std::vector<double> w(leaves.size());
    for (size_t j = 0; j < leaves.size(); ++j) { at[j] = (uint32_t)j; w[j] = oc_weight((int64_t)leaves[j].end - leaves[j].start, power); }
    std::sort(at.begin(), at.end(), [&](uint32_t a, uint32_t b) {
        const uint32_t ca = leaves[a].end - leaves[a].start, cb = leaves[b].end - leaves[b].start;
        if (w[a] != w[b]) return w[a] > w[b];
        if (ca != cb) return ca > cb;
        return first[a] < first[b];
    });
    if ((int64_t)at.size() > target) at.resize((size_t)target);
    return at;
}

}  // namespace gs360
