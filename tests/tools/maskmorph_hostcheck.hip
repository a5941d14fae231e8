// maskmorph_hostcheck.hip -- the mask-finishing kernels' arithmetic (csrc/gs360_maskmorph.hip, MSK-SPEC v1) stepped lane by lane on the
// host.  A CPU-only stand-alone program: it includes the kernels' source, calls the host-callable per-lane functions in the order and
// with the tile, row and dword numbers the kernels use (the stepping is mask_hoststep.h's, the geometry csrc/gs360_maskplane.h's), and
// allocates the raw mask, the add layer, the image, the planes, the element rows, every staged band and the output at their exact
// sizes, so that a build with -fsanitize=address,undefined (tests/test_maskmorph_hostcheck.py) turns any read or write outside a
// buffer into a failure.  Usage: maskmorph_hostcheck IN.bin OUT.bin; IN = 16 int32 (H, W, thresh, close kw, close kh, expand kw,
// expand kh, fuse, spread, kind, invert, has raw, has add, 0...), the close rows, the expand rows (pairs of int32), the raw mask, the
// add layer, the image (H x W x 3, unless kind 0); OUT = the output rows.  Prints the count and the output's FNV-1a checksum.
#include "mask_hoststep.h"

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
    Plane a((size_t)H * J.pw, 0xA5A5A5A5u), b((size_t)H * J.pw, 0xA5A5A5A5u);   // exact: no slack behind a plane
    // mk_pack_kernel
    step_words(H, W, kMkPackTile, [&](int y, int x) { return mk_nibble(J.src, J.src_stride, W, J.thresh, y, x); },
               [&](int y, int w, uint32_t word) { a[(size_t)y * J.pw + w] = word; });
    Plane *cur = &a, *other = &b;
    if (ckh) {
        morph(J, *cur, *other, crow, ckw, ckh, 0); std::swap(cur, other);
        morph(J, *cur, *other, crow, ckw, ckh, kMkCompIn | kMkCompOut); std::swap(cur, other);
    }
    if (ekh) { morph(J, *cur, *other, erow, ekw, ekh, 0); std::swap(cur, other); }
    if (J.f) {                                            // mk_fuse_kernel: the copy, then every item of the fills
        J.in = cur->data(); J.out = other->data();
        for (int64_t q = 0; q < mk_plane_items(J); ++q) J.out[q] = J.in[q];
        for (int64_t q = 0; q < mk_fuse_items(J); ++q) mk_fuse_item(J, (int)q);
        std::swap(cur, other);
    }
    // mk_finish_kernel, phase 0 then 1
    J.out = cur->data();
    uint32_t count = 0;
    step_words(H, W, kMkCountTile,
               [&](int y, int x) {
                   const uint32_t nib = mk_plane_nibble(J.out, J.pw, y, x) | mk_nibble(J.add, J.add_stride, W, 0, y, x);
                   count += (uint32_t)mk_popc(nib);
                   return nib;
               },
               [&](int y, int w, uint32_t word) { if (J.add) J.out[(size_t)y * J.pw + w] = word; });
    const MkTile t = mk_output_tile(kind);
    for (int y = 0; y < H; ++y)
        for (int x0 = 0; x0 < W; x0 += t.w)
            for (int lane = 0; lane < kMkThreads; ++lane) {
                if (kind == GS360_MASK_OUT_MASK) mk_compose_mask4(J, y, x0 + 4 * lane);
                else if (x0 + lane < W) mk_compose(J, y, x0 + lane, count);
            }
    uint64_t h = 1469598103934665603ull;
    for (uint8_t v : dst) h = (h ^ v) * 1099511628211ull;
    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(dst.data(), 1, dst.size(), o) != dst.size()) return 2;
    fclose(o);
    printf("%u %016llx\n", count, (unsigned long long)h);
    return 0;
}
