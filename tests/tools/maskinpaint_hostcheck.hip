// maskinpaint_hostcheck.hip -- the inpaint stage's arithmetic (csrc/gs360_maskinpaint.hip, MSK-INPAINT v1) stepped lane by lane on the
// host.  A CPU-only stand-alone program: it includes the kernels' source, calls the host-callable per-lane functions in the order and
// with the tile, row and item numbers the kernels use (the geometry of csrc/gs360_maskplane.h; a barrier is the end of a lane loop,
// an LDS array a vector of its size, lanes one after another are one valid schedule of the atomics), and allocates every plane, table
// and list at its exact size, so that a build with -fsanitize=address,undefined (tests/test_maskinpaint_hostcheck.py) turns any read
// or write outside a buffer into a failure.  Usage: maskinpaint_hostcheck IN.bin OUT.bin [reverse]; IN = 4 int32 (H, W, radius,
// n_off), n_off (dy, dx) pairs (int32), n_off |r| and n_off 1 / |r|^2 (float32), the image (H x W x 3), F (H x W); OUT = the filled
// image.  `reverse` scatters the workgroups last to first: another order inside every level.  Prints K, the pixels listed and the
// error word.
#include "../../360cam-pgm-3dgs-tools_amd/csrc/gs360_maskinpaint.hip"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace gs360;

static bool read_all(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    FILE* f = argc >= 3 ? fopen(argv[1], "rb") : nullptr;
    int32_t hd[4];
    if (!f || !read_all(f, hd, sizeof(hd))) return 2;
    const int H = hd[0], W = hd[1], n_off = hd[3];
    const bool reverse = argc >= 4;
    if (H < 1 || W < 1 || n_off < 1 || n_off > kMiMaxOffsets) return 2;
    const size_t px = (size_t)H * W;
    std::vector<int32_t> off(2 * (size_t)n_off);
    std::vector<float> rlen(n_off), inv2(n_off);
    std::vector<uint8_t> img(px * 3), fill(px);
    if (!read_all(f, off.data(), off.size() * 4) || !read_all(f, rlen.data(), rlen.size() * 4) || !read_all(f, inv2.data(), inv2.size() * 4) ||
        !read_all(f, img.data(), img.size()) || !read_all(f, fill.data(), fill.size())) return 2;
    fclose(f);

    // every buffer at its exact size: no slack behind a plane or the list
    std::vector<uint16_t> vert(px, 0xA5A5), lev(px, 0xA5A5);
    std::vector<float> dist(px, -1.0f);
    std::vector<MiHead> head(1);
    memset(head.data(), 0, sizeof(MiHead));
    uint32_t levels = 0;

    MiLaunch L;
    memset(&L, 0, sizeof(L));
    L.n_jobs = 1; L.head = head.data(); L.levels = &levels;
    MiJob& J = L.job[0];
    J.img = img.data(); J.fill = fill.data(); J.img_stride = 3 * (int64_t)W; J.fill_stride = W;
    J.vert = vert.data(); J.lev = lev.data(); J.dist = dist.data();
    J.off = off.data(); J.rlen = rlen.data(); J.inv2 = inv2.data();
    J.H = H; J.W = W; J.n_off = n_off;

    // mi_cols_kernel: an item per column, the count tail
    for (int64_t x = 0; x < mi_cols_items(J); ++x) head[0].filled[0] += mi_cols_lane(J, (int)x);
    // mi_rows_kernel: per workgroup the LDS histogram, the flush of its bins and of its highest level
    const int tiles_x = (W + kMiRowTile.w - 1) / kMiRowTile.w;
    for (int y = 0; y < H; ++y)
        for (int tx = 0; tx < tiles_x; ++tx) {
            std::vector<uint32_t> hist(kMiFar + 1, 0);
            for (int lane = 0; lane < kMiThreads; ++lane) {
                const int x = tx * kMiRowTile.w + lane;
                if (x < W) {
                    const int lv = mi_rows_lane(J, y, x, mi_full(J, L.head, 0));
                    if (lv) ++hist[lv];
                }
            }
            for (int i = 0; i <= kMiFar; ++i)
                if (hist[i]) {
                    mk_atomic_add(head[0].hist + i, hist[i]);
                    mk_atomic_max(&levels, (uint32_t)i);
                }
        }
    // mi_scan_kernel
    {
        std::vector<uint32_t> part(kMiThreads);
        for (int lane = 0; lane < kMiThreads; ++lane) part[lane] = mi_scan_sum(L.head, lane);
        uint32_t base = 0;
        for (int i = 0; i < kMiThreads; ++i) { const uint32_t n = part[i]; part[i] = base; base += n; }
        for (int lane = 0; lane < kMiThreads; ++lane) mi_scan_write(L.head, lane, part[lane]);
    }
    // the list holds exactly the pixels of the levels 1 .. kMiMaxLevel
    uint32_t listed = 0;
    for (int i = 1; i <= kMiMaxLevel; ++i) listed += head[0].hist[i];
    std::vector<uint32_t> list(listed, 0xA5A5A5A5u);
    L.list = list.data(); L.list_cap = listed;
    // mi_scatter_kernel: ranks, barrier, the runs, barrier, the entries
    for (int t = 0; t < H * tiles_x; ++t) {
        const int tile = reverse ? H * tiles_x - 1 - t : t, y = tile / tiles_x, tx = tile - y * tiles_x;
        std::vector<uint32_t> cnt(kMiFar + 1, 0), run(kMiFar + 1, 0), rank(kMiThreads, 0);
        std::vector<int> lv(kMiThreads, 0);
        for (int lane = 0; lane < kMiThreads; ++lane) lv[lane] = mi_scatter_rank(J, y, tx * kMiRowTile.w + lane, cnt.data(), &rank[lane]);
        for (int i = 0; i <= kMiFar; ++i)
            if (cnt[i]) run[i] = mk_atomic_fetch_add(head[0].cursor + i, cnt[i]);
        for (int lane = 0; lane < kMiThreads; ++lane)
            if (lv[lane]) mi_scatter_put(L, J, y, tx * kMiRowTile.w + lane, lv[lane], run[lv[lane]] + rank[lane]);
    }
    // mi_fill_kernel, one launch per level, unless the call would refuse the job
    if (!head[0].hist[kMiFar])
        for (int level = 1; level <= kMiMaxLevel; ++level) {
            L.level = level; L.items = head[0].hist[level];
            for (int64_t tile = 0; tile < mk_item_tiles(L.items); ++tile)
                for (int lane = 0; lane < kMiThreads; ++lane) {
                    const uint32_t i = (uint32_t)tile * kMiThreads + lane;
                    if (i < L.items) mi_fill_item(L, i);
                }
        }

    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(img.data(), 1, img.size(), o) != img.size()) return 2;
    fclose(o);
    printf("%u %u %u\n", levels, listed, head[0].err);
    return 0;
}
