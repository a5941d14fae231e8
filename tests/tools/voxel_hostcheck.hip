// voxel_hostcheck.hip -- the per-lane arithmetic of the voxel downsampling (csrc/gs360_voxel.h, VOX-SPEC v1) stepped on the host.
// A CPU-only stand-alone program: it includes the kernels' header and calls its host-callable functions -- the key of every point
// (vx_point_key), then, over a stable sort of the (key, index) pairs and the segment starts found here, a lane's pick of every
// segment (vx_pick_lane, with vx_center and cloud_dist2) -- with every array allocated at its exact size, so that a build with
// -fsanitize=address,undefined (tests/test_voxel_hostcheck.py) turns any read or write outside a buffer, and any undefined shift or
// conversion, into a failure.  Usage: voxel_hostcheck IN.bin OUT.bin; IN = n (int64), strategy, shift[0], shift[1], 0 (int32), the
// cloud's minimum and (float) voxel (4 float32), kmax (3 uint64), the n x 3 float32 points; OUT = k picks (uint32).  Prints k and the
// number of keys outside their bounds.
#include "../../360cam-pgm-3dgs-tools_amd/csrc/gs360_voxel.h"
#include <algorithm>
#include <cstdio>
#include <numeric>
#include <vector>
using namespace gs360;

static bool read_all(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    VxLaunch L = {};
    int32_t head[4];
    float fl[4];
    if (!read_all(f, &L.n, 8) || !read_all(f, head, 16) || !read_all(f, fl, 16) || !read_all(f, L.kmax, 24) || L.n < 1) return 3;
    L.strategy = head[0]; L.shift[0] = head[1]; L.shift[1] = head[2];
    for (int a = 0; a < 3; ++a) L.lo[a] = fl[a];
    L.v = fl[3];
    std::vector<float> xyz(3 * (size_t)L.n);
    if (!read_all(f, xyz.data(), xyz.size() * 4)) return 3;
    fclose(f);
    L.xyz = xyz.data();
    std::vector<uint64_t> keys((size_t)L.n), sorted((size_t)L.n);
    long bad = 0;
    for (int64_t p = 0; p < L.n; ++p) bad += !vx_point_key(L, xyz[3 * p], xyz[3 * p + 1], xyz[3 * p + 2], &keys[p]);
    std::vector<uint32_t> idx((size_t)L.n), starts;
    std::iota(idx.begin(), idx.end(), 0u);
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
    for (int64_t p = 0; p < L.n; ++p) {
        sorted[p] = keys[idx[p]];
        if (p == 0 || sorted[p] != sorted[p - 1]) starts.push_back((uint32_t)p);
    }
    L.keys = sorted.data(); L.idx = idx.data();
    std::vector<uint32_t> pick(starts.size());
    for (size_t g = 0; g < starts.size(); ++g) {
        const int64_t s = starts[g], e = g + 1 < starts.size() ? (int64_t)starts[g + 1] : L.n;
        pick[g] = vx_pick_lane(L, s, e, sorted[s]);
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(pick.data(), 4, pick.size(), o) != pick.size()) return 3;
    fclose(o);
    printf("%zu %ld\n", pick.size(), bad);
    return 0;
}
