// mask_hoststep.h -- what the two mask host checks (maskmorph_hostcheck.hip, maskshadow_hostcheck.hip) share: the morph kernel's source
// and the host-side stepping of the launches both of them take.  A barrier becomes the end of a lane loop, a shuffle among eight
// lanes a loop over them; tiles and lanes come from the geometry the kernels and the glue use (csrc/gs360_maskplane.h).
#pragma once
#include "../../360cam-pgm-3dgs-tools_amd/csrc/gs360_maskmorph.hip"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace gs360;
typedef std::vector<uint32_t> Plane;

static bool read_all(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

// mk_morph_kernel over every tile of the plane: the kernel's three per-lane functions for all 256 lanes; the band is staged into a
// buffer of exactly the dwords the kernel stages, so that the sanitizer guards the band's end
static void morph(MkJob J, const Plane& in, Plane& out, const std::vector<int32_t>& rows, int kw, int kh, int flags) {
    J.in = in.data(); J.out = out.data(); J.spans = rows.data();
    J.kh = kh; J.ax = kw / 2; J.ay = kh / 2; J.halo = mk_element_halo(rows.data(), kw, kh); J.flags = flags;
    for (int y0 = 0; y0 < J.H; y0 += kMkMorphTile.h)
        for (int w0 = 0; w0 < J.pw; w0 += kMkMorphTile.w) {
            std::vector<MkAcc> acc(kMkThreads, MkAcc{0, 0, 0, 0});
            for (int i0 = 0; i0 < kh; i0 += kMkBand) {
                if (mk_band_dwords(J, i0) > kMkStageRows * kMkStageW) exit(4);       // the kernel's LDS array
                Plane stage(mk_band_dwords(J, i0));
                for (int lane = 0; lane < kMkThreads; ++lane) mk_morph_stage(J, y0, w0, i0, lane, stage.data());
                for (int lane = 0; lane < kMkThreads; ++lane) mk_morph_band(J, w0, i0, lane, stage.data(), acc[lane]);
            }
            for (int lane = 0; lane < kMkThreads; ++lane) mk_morph_store(J, y0, w0, lane, acc[lane]);
        }
}

// a tiled step whose lanes take four pixels each and gather eight lanes' nibbles into a word (mk_gather8, mk_store_word): every lane
// of every tile of an H x W plane.  nib(y, x): the nibble of the lane at column x; put(y, w, word): the first lane's store to dword w
template <class Nib, class Put>
static void step_words(int H, int W, MkTile t, Nib nib, Put put) {
    const int pw = (W + 31) / 32;
    for (int y = 0; y < H; ++y)
        for (int x0 = 0; x0 < W; x0 += t.w)
            for (int x = x0; x < x0 + 4 * kMkThreads; x += 32) {
                uint32_t word = 0;
                for (int l = 0; l < 8; ++l) word |= nib(y, x + 4 * l) << (4 * l);
                if ((x >> 5) < pw) put(y, x >> 5, word);
            }
}
