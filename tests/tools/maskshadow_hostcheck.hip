// maskshadow_hostcheck.hip -- the shadow estimate's arithmetic (csrc/gs360_maskshadow.hip, MSK-SHADOW v1) stepped lane by lane on the
// host.  A CPU-only stand-alone program: it includes the kernels' sources, calls the host-callable per-lane functions in the order and
// with the tile, row and item numbers the kernels use (mask_hoststep.h and the geometry of csrc/gs360_maskplane.h; a ballot is a loop over
// the wave's lanes, lanes one after another are one valid schedule of the label kernels), and allocates every plane, table and staged tile at its exact
// size, so that a build with -fsanitize=address,undefined (tests/test_maskshadow_hostcheck.py) turns any read or write outside a
// buffer into a failure.  Usage: maskshadow_hostcheck IN.bin OUT.bin; IN = 16 int32 (H, W, thresh, close kw, kh, radius, sat_max,
// min_area, near kw, kh, shadow-close kw, kh, open kw, kh, has raw, 0), t and delta_min (float32), the four elements' rows (pairs of
// int32), radius + 1 weights (float32), 256 divisors (int32), the raw mask, the image; OUT = P, C0, C1, C2, clean (a byte of 0 / 1
// per pixel) and M (0 / 255).  Prints count(P), count(M) and the error word.
#include "mask_hoststep.h"
#include "../../360cam-pgm-3dgs-tools_amd/csrc/gs360_maskshadow.hip"

// the three label kernels over plane `a` (or its complement)
static void label(MsJob& J, const Plane& a, int conn, int flags, uint32_t* err) {
    J.a = a.data(); J.flags = flags;
    const int64_t dwords = mk_plane_items(J);
    for (int64_t q = 0; q < dwords; ++q) ms_label_init(J, q);
    for (int64_t q = 0; q < dwords; ++q) conn == 8 ? ms_label_merge<8>(J, q, err) : ms_label_merge<4>(J, q, err);
    for (int64_t q = 0; q < dwords; ++q) ms_label_flatten(J, q, err);
}

static void put_plane(std::vector<uint8_t>& out, const Plane& p, int H, int W, int pw) {
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) out.push_back(mk_bit(p.data(), pw, y, x));
}

int main(int argc, char** argv) {
    FILE* f = argc >= 3 ? fopen(argv[1], "rb") : nullptr;
    int32_t hd[16];
    float fl[2];
    if (!f || !read_all(f, hd, sizeof(hd)) || !read_all(f, fl, sizeof(fl))) return 2;
    const int H = hd[0], W = hd[1], r = hd[5], pw = (W + 31) / 32;
    const int kw[4] = {hd[3], hd[8], hd[10], hd[12]}, kh[4] = {hd[4], hd[9], hd[11], hd[13]};
    std::vector<int32_t> rows[4];
    for (int e = 0; e < 4; ++e) {
        rows[e].resize(2 * (size_t)kh[e]);
        if (!read_all(f, rows[e].data(), rows[e].size() * 4)) return 2;
    }
    std::vector<float> weights(r + 1);
    std::vector<int32_t> sdiv(256);
    std::vector<uint8_t> raw(hd[14] ? (size_t)H * W : 0), img((size_t)H * W * 3);
    if (!read_all(f, weights.data(), weights.size() * 4) || !read_all(f, sdiv.data(), 1024) || !read_all(f, raw.data(), raw.size()) ||
        !read_all(f, img.data(), img.size())) return 2;
    fclose(f);

    // every buffer at its exact size: no slack behind a plane
    const size_t dwords = (size_t)H * pw;
    Plane P(dwords, 0xA5A5A5A5u), C0(dwords, 0xA5A5A5A5u), C1(dwords, 0xA5A5A5A5u), C2(dwords, 0xA5A5A5A5u), clean(dwords, 0xA5A5A5A5u),
        sat(dwords, 0xA5A5A5A5u), T0(dwords, 0xA5A5A5A5u), T1(dwords, 0xA5A5A5A5u);
    std::vector<uint8_t> gray((size_t)H * 32 * pw, 0xA5), dst((size_t)H * W, 0xA5);
    std::vector<float> mid((size_t)H * W, -1.0f);
    std::vector<int32_t> lab((size_t)H * W, 0x5A5A5A5A);
    std::vector<uint32_t> area((size_t)H * W, 0);
    uint32_t err = 0, count_p = 0, count_m = 0;

    MkJob K;
    memset(&K, 0, sizeof(K));
    K.src = raw.empty() ? nullptr : raw.data(); K.src_stride = W;
    K.H = H; K.W = W; K.pw = pw; K.thresh = hd[2];
    MsJob J;
    memset(&J, 0, sizeof(J));
    J.img = img.data(); J.img_stride = 3 * (int64_t)W; J.dst = dst.data(); J.dst_stride = W;
    J.gray = gray.data(); J.mid = mid.data(); J.lab = lab.data(); J.area = area.data();
    J.k = weights.data(); J.sdiv = sdiv.data();
    J.H = H; J.W = W; J.pw = pw; J.r = r; J.t = fl[0]; J.delta_min = fl[1]; J.sat_max = hd[6];
    J.th2 = 2u * (uint32_t)std::max(1, hd[7]);

    // mk_pack_kernel, the close
    Plane& packed = kh[0] ? T0 : P;
    step_words(H, W, kMkPackTile, [&](int y, int x) { return mk_nibble(K.src, K.src_stride, W, K.thresh, y, x); },
               [&](int y, int w, uint32_t word) { packed[(size_t)y * pw + w] = word; });
    if (kh[0]) {
        morph(K, T0, T1, rows[0], kw[0], kh[0], 0);
        morph(K, T1, P, rows[0], kw[0], kh[0], kMkCompIn | kMkCompOut);
    }
    for (uint32_t v : P) count_p += (uint32_t)mk_popc(v);

    // ms_pixel_kernel
    step_words(H, W, kMsPixelTile,
               [&](int y, int x) {
                   uint32_t gray4, nib;
                   ms_pixel4(J, y, x, &gray4, &nib);
                   if (x < 32 * pw) memcpy(gray.data() + (size_t)y * 32 * pw + x, &gray4, 4);
                   return nib;
               },
               [&](int y, int w, uint32_t word) { sat[(size_t)y * pw + w] = word; });
    // ms_blur_rows_kernel: stage, barrier, outputs
    for (int y = 0; y < H; ++y)
        for (int x0 = 0; x0 < W; x0 += kMsRowsTile.w) {
            const int floats = ms_skew(ms_rows_len(J, x0) + 2 * r - 1) + 1;
            if (floats > kMsRowStage) return 4;               // the kernel's LDS array
            std::vector<float> stage(floats, -1.0f);
            for (int lane = 0; lane < kMsThreads; ++lane) ms_rows_stage(J, y, x0, lane, stage.data());
            for (int lane = 0; lane < kMsThreads; ++lane) ms_rows_lane(J, y, x0, lane, stage.data());
        }
    // ms_blur_cols_kernel: stage, barrier, per wave and chunk the lanes' bits and the ballot
    J.a = sat.data();
    for (int y0 = 0; y0 < H; y0 += kMsColsTile.h)
        for (int x0 = 0; x0 < W; x0 += kMsColsTile.w) {
            if (ms_cols_rows(J, y0) > kMsColRows + 2 * r) return 4;   // the launch's dynamic LDS
            std::vector<float> stage((size_t)ms_cols_rows(J, y0) * kMsColW, -1.0f);
            for (int lane = 0; lane < kMsThreads; ++lane) ms_cols_stage(J, y0, x0, lane, stage.data());
            for (int wave = 0; wave < 4; ++wave)
                for (int chunk = 0; chunk < kMsColRows / 4 / kMsOut; ++chunk) {
                    const int c0 = wave * (kMsColRows / 4) + chunk * kMsOut;
                    if (y0 + c0 >= H) break;
                    uint32_t bits[kMsColW];
                    for (int l = 0; l < kMsColW; ++l) bits[l] = ms_cols_lane(J, y0, x0, wave * kMsColW + l, c0, stage.data());
                    for (int k = 0; k < kMsOut && y0 + c0 + k < H; ++k)
                        for (int half = 0; half < 2; ++half) {
                            uint32_t word = 0;
                            for (int b = 0; b < 32; ++b) word |= ((bits[32 * half + b] >> k) & 1u) << b;
                            if ((x0 >> 5) + half < pw) C0[(size_t)(y0 + c0 + k) * pw + (x0 >> 5) + half] = word;
                        }
                }
        }

    // the merge: near region, plane logic, close, open
    morph(K, P, T0, rows[1], kw[1], kh[1], 0);
    for (size_t q = 0; q < dwords; ++q) C1[q] = C0[q] & T0[q] & ~P[q];
    morph(K, C1, T0, rows[2], kw[2], kh[2], 0);
    morph(K, T0, T1, rows[2], kw[2], kh[2], kMkCompIn | kMkCompOut);
    morph(K, T1, T0, rows[3], kw[3], kh[3], kMkCompIn | kMkCompOut);
    morph(K, T0, C2, rows[3], kw[3], kh[3], 0);
    // O and G = ~O (in T1)
    label(J, C2, 4, kMsComplement, &err);
    for (int64_t q = 0; q < ms_border_items(J); ++q) ms_border(J, q);
    for (int y = 0; y < H; ++y)
        for (int x0 = 0; x0 < W; x0 += kMsFillTile.w)
            for (int x = x0; x < x0 + kMsThreads; x += 32) {                          // half a wave's ballot
                uint32_t word = 0;
                for (int b = 0; b < 32; ++b) word |= (uint32_t)(x + b < W && ms_fill_bit(J, y, x + b)) << b;
                if ((x >> 5) < pw) T1[(size_t)y * pw + (x >> 5)] = word;
            }
    // the components of G, their areas, the selection
    std::fill(area.begin(), area.end(), 0u);
    label(J, T1, 8, 0, &err);
    for (int64_t q = 0; q < ms_area_items(J); ++q) ms_area_lane(J, q, &err);
    J.a = T1.data(); J.b = P.data();
    step_words(H, W, kMsSelectTile,
               [&](int y, int x) {
                   uint32_t c, m;
                   ms_select4(J, y, x, &c, &m);
                   count_m += (uint32_t)mk_popc(m);
                   return c;
               },
               [&](int y, int w, uint32_t word) { clean[(size_t)y * pw + w] = word; });

    std::vector<uint8_t> out;
    for (const Plane* p : {&P, &C0, &C1, &C2, &clean}) put_plane(out, *p, H, W, pw);
    out.insert(out.end(), dst.begin(), dst.end());
    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(out.data(), 1, out.size(), o) != out.size()) return 2;
    fclose(o);
    printf("%u %u %u\n", count_p, count_m, err);
    return 0;
}
