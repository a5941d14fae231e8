// maskmorph_hostcheck.hip -- the mask-finishing kernels' arithmetic (csrc/gs360_maskmorph.hip, MSK-SPEC v1) stepped lane by lane on the
// host.  A CPU-only stand-alone program: it includes the kernels' source, calls the host-callable per-lane functions in the order and
// with the tile, row and dword numbers the kernels use (barriers become loop boundaries, a shuffle among eight lanes a loop over them), and
// allocates the raw mask, the add layer, the image, the planes, the element rows, every staged band and the output at their exact
// sizes, so that a build with -fsanitize=address,undefined (tests/test_maskmorph_hostcheck.py) turns any read or write outside a
// buffer into a failure.  Usage: maskmorph_hostcheck IN.bin OUT.bin; IN = 16 int32 (H, W, thresh, close kw, close kh, expand kw,
// expand kh, fuse, spread, kind, invert, has raw, has add, 0...), the close rows, the expand rows (pairs of int32), the raw mask, the
// add layer, the image (H x W x 3, unless kind 0); OUT = the output rows.  Prints the count and the output's FNV-1a checksum.
#include "../../360cam-pgm-3dgs-tools_amd/csrc/gs360_maskmorph.hip"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace gs360;

static bool read_all(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

// mk_morph_kernel over every tile of the plane: the kernel's three per-lane functions for all 256 lanes, a barrier being the end of a
// lane loop; the band is staged into a buffer of exactly the dwords the kernel stages
static void morph(MkJob J, const std::vector<uint32_t>& in, std::vector<uint32_t>& out, const std::vector<int32_t>& rows, int kw, int kh, int flags) {
    int reach = 0;
    for (int i = 0; i < kh; ++i)
        if (rows[2 * i + 1] > rows[2 * i]) reach = std::max({reach, std::abs(rows[2 * i] - kw / 2), std::abs(rows[2 * i + 1] - 1 - kw / 2)});
    J.in = in.data(); J.out = out.data(); J.spans = rows.data();
    J.kh = kh; J.ax = kw / 2; J.ay = kh / 2; J.halo = reach / 32 + 2; J.flags = flags;
    for (int y0 = 0; y0 < J.H; y0 += kMkTileR)
        for (int w0 = 0; w0 < J.pw; w0 += kMkTileW) {
            std::vector<MkAcc> acc(kMkThreads, MkAcc{0, 0, 0, 0});
            for (int i0 = 0; i0 < kh; i0 += kMkBand) {
                if (mk_band_dwords(J, i0) > kMkStageRows * kMkStageW) exit(4);       // the kernel's LDS array
                std::vector<uint32_t> stage(mk_band_dwords(J, i0));                  // exact: the sanitizer guards the band's end
                for (int lane = 0; lane < kMkThreads; ++lane) mk_morph_stage(J, y0, w0, i0, lane, stage.data());
                for (int lane = 0; lane < kMkThreads; ++lane) mk_morph_band(J, w0, i0, lane, stage.data(), acc[lane]);
            }
            for (int lane = 0; lane < kMkThreads; ++lane) mk_morph_store(J, y0, w0, lane, acc[lane]);
        }
}

int main(int argc, char** argv) {
    FILE* f = argc >= 3 ? fopen(argv[1], "rb") : nullptr;
    int32_t hd[16];
    if (!f || !read_all(f, hd, sizeof(hd))) return 2;
    const int H = hd[0], W = hd[1], ckw = hd[3], ckh = hd[4], ekw = hd[5], ekh = hd[6], kind = hd[9];
    const int out_c = kind == GS360_MASK_OUT_MASK ? 1 : kind == GS360_MASK_OUT_RGBA ? 4 : 3;
    std::vector<int32_t> crow(2 * (size_t)ckh), erow(2 * (size_t)ekh);
    std::vector<uint8_t> raw(hd[11] ? (size_t)H * W : 0), add(hd[12] ? (size_t)H * W : 0), img(out_c > 1 ? (size_t)H * W * 3 : 0);
    if (!read_all(f, crow.data(), crow.size() * 4) || !read_all(f, erow.data(), erow.size() * 4) || !read_all(f, raw.data(), raw.size()) ||
        !read_all(f, add.data(), add.size()) || !read_all(f, img.data(), img.size())) return 2;
    fclose(f);
    std::vector<uint8_t> dst((size_t)H * W * out_c, 0xA5);
    MkJob J;
    memset(&J, 0, sizeof(J));
    J.src = raw.empty() ? nullptr : raw.data(); J.add = add.empty() ? nullptr : add.data(); J.img = img.empty() ? nullptr : img.data();
    J.dst = dst.data();
    J.src_stride = J.add_stride = W; J.img_stride = 3 * (int64_t)W; J.dst_stride = (int64_t)W * out_c;
    J.H = H; J.W = W; J.pw = (W + 31) / 32; J.thresh = hd[2];
    J.f = hd[7]; J.s = hd[8]; J.kind = kind; J.invert = hd[10];
    std::vector<uint32_t> a((size_t)H * J.pw, 0xA5A5A5A5u), b((size_t)H * J.pw, 0xA5A5A5A5u);   // exact: no slack behind a plane
    // mk_pack_kernel: a lane's four pixels as a nibble, eight lanes' nibbles as a dword stored by the first of them
    const int lanes_x = (W + 4 * kMkThreads - 1) / (4 * kMkThreads) * kMkThreads;
    for (int y = 0; y < H; ++y)
        for (int l0 = 0; l0 < lanes_x; l0 += 8) {
            uint32_t word = 0;
            for (int l = 0; l < 8; ++l) word |= mk_nibble(J.src, J.src_stride, W, J.thresh, y, 4 * (l0 + l)) << (4 * l);
            if (l0 / 8 < J.pw) a[(size_t)y * J.pw + l0 / 8] = word;
        }
    std::vector<uint32_t>*cur = &a, *other = &b;
    if (ckh) {
        morph(J, *cur, *other, crow, ckw, ckh, 0); std::swap(cur, other);
        morph(J, *cur, *other, crow, ckw, ckh, kMkCompIn | kMkCompOut); std::swap(cur, other);
    }
    if (ekh) { morph(J, *cur, *other, erow, ekw, ekh, 0); std::swap(cur, other); }
    if (J.f) {                                            // mk_fuse_kernel: the copy, then every item of the fills
        J.in = cur->data(); J.out = other->data();
        for (size_t q = 0; q < cur->size(); ++q) J.out[q] = J.in[q];
        for (int q = 0; q < mk_fuse_items(J); ++q) mk_fuse_item(J, q);
        std::swap(cur, other);
    }
    // mk_finish_kernel, phase 0 then 1
    J.out = cur->data();
    uint32_t count = 0;
    for (int y = 0; y < H; ++y)
        for (int l0 = 0; l0 < lanes_x; l0 += 8) {
            uint32_t word = 0;
            for (int l = 0; l < 8; ++l)
                word |= (mk_plane_nibble(J.out, J.pw, y, 4 * (l0 + l)) | mk_nibble(J.add, J.add_stride, W, 0, y, 4 * (l0 + l))) << (4 * l);
            if (J.add && l0 / 8 < J.pw) J.out[(size_t)y * J.pw + l0 / 8] = word;
            count += (uint32_t)__builtin_popcount(word);
        }
    for (int y = 0; y < H; ++y) {
        if (kind == GS360_MASK_OUT_MASK)
            for (int l = 0; l < lanes_x; ++l) mk_compose_mask4(J, y, 4 * l);
        else
            for (int x = 0; x < W; ++x) mk_compose(J, y, x, count);
    }
    uint64_t h = 1469598103934665603ull;
    for (uint8_t v : dst) h = (h ^ v) * 1099511628211ull;
    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(dst.data(), 1, dst.size(), o) != dst.size()) return 2;
    fclose(o);
    printf("%u %016llx\n", count, (unsigned long long)h);
    return 0;
}
