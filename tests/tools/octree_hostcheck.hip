// octree_hostcheck.hip -- the adaptive octree sampling (csrc/gs360_octree.h, OCT-SPEC v1) stepped on the host.  A CPU-only stand-alone
// program: it calls the header's host-callable functions -- the path code of every point (oc_point_code), over a stable sort of the
// (code, index) pairs the divergence level of every sorted position (oc_level), the split loop over counts (oc_walk), the leaves'
// ordinals and the stable sort by them, a lane's pick of every leaf (oc_pick_lane, with oc_center and cloud_dist2) and the selection
// (oc_select) -- with every array allocated at its exact size, so that a build with -fsanitize=address,undefined
// (tests/test_octree_hostcheck.py) turns any read or write outside a buffer, and any undefined shift or conversion, into a failure.
// Usage: octree_hostcheck IN.bin OUT.bin; IN = n, target (int64), strategy, 0 (int32), weight power, smallest voxel (0: none), cube
// size (float64), the cube's corner and a pad (4 float32), the n x 3 float32 points; OUT = k picks (uint32).  Prints k, the number
// of leaves and the largest code in hex.
#include "../../360cam-pgm-3dgs-tools_amd/csrc/gs360_octree.h"
#include <cstdio>
#include <numeric>
using namespace gs360;

static bool read_all(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    OcLaunch L = {};
    int64_t nt[2];
    int32_t head[2];
    double dbl[3];
    float fl[4];
    if (!read_all(f, nt, 16) || !read_all(f, head, 8) || !read_all(f, dbl, 24) || !read_all(f, fl, 16) || nt[0] < 2 || nt[1] < 1 || nt[1] >= nt[0]) return 3;
    const int64_t n = nt[0], target = nt[1];
    const double power = dbl[0], min_voxel = dbl[1], cube_size = dbl[2];
    L.n = n; L.strategy = head[0];
    for (int a = 0; a < 3; ++a) L.lo[a] = fl[a];
    for (int l = 0; l <= kOcDepth; ++l) L.half[l] = (float)(std::ldexp(cube_size, -l) * 0.5);
    std::vector<float> xyz(3 * (size_t)n);
    if (!read_all(f, xyz.data(), xyz.size() * 4)) return 3;
    fclose(f);
    L.xyz = xyz.data();
    std::vector<uint64_t> codes((size_t)n);
    for (int64_t p = 0; p < n; ++p) codes[p] = oc_point_code(L, xyz[3 * p], xyz[3 * p + 1], xyz[3 * p + 2]);
    std::vector<uint32_t> idx((size_t)n);
    std::iota(idx.begin(), idx.end(), 0u);
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return codes[a] < codes[b]; });
    std::vector<uint8_t> lvl((size_t)n);
    lvl[0] = 0;
    for (int64_t p = 1; p < n; ++p) lvl[p] = oc_level(codes[idx[p - 1]], codes[idx[p]]);
    std::vector<OcLeaf> leaves;
    oc_walk(lvl.data(), n, target, power, min_voxel, cube_size, &leaves);
    std::sort(leaves.begin(), leaves.end(), [](const OcLeaf& a, const OcLeaf& b) { return a.start < b.start; });
    std::vector<uint32_t> ord((size_t)n), grouped((size_t)n);
    for (size_t j = 0; j < leaves.size(); ++j)
        for (uint32_t p = leaves[j].start; p < leaves[j].end; ++p) ord[idx[p]] = (uint32_t)j;
    std::iota(grouped.begin(), grouped.end(), 0u);
    std::stable_sort(grouped.begin(), grouped.end(), [&](uint32_t a, uint32_t b) { return ord[a] < ord[b]; });
    L.idx = grouped.data();
    std::vector<uint32_t> pick(leaves.size()), first(leaves.size());
    for (size_t j = 0; j < leaves.size(); ++j) {
        pick[j] = oc_pick_lane(L, leaves[j].start, leaves[j].end, leaves[j].depth);
        first[j] = grouped[leaves[j].start];
    }
    const std::vector<uint32_t> kept = oc_select(leaves, first.data(), target, power);
    std::vector<uint32_t> out(kept.size());
    for (size_t j = 0; j < kept.size(); ++j) out[j] = pick[kept[j]];
    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(out.data(), 4, out.size(), o) != out.size()) return 3;
    fclose(o);
    printf("%zu %zu %llx\n", out.size(), leaves.size(), (unsigned long long)*std::max_element(codes.begin(), codes.end()));
    return 0;
}
