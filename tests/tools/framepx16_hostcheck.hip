// framepx16_hostcheck.hip -- the shared per-pixel steps of the FrameSelector passes (csrc/gs360_framepx.h) on 16-bit samples, stepped
// on the host.  A CPU-only stand-alone program: it calls the host-callable steps -- gray_of<C, uint16_t> (the gray at full depth),
// gray8_of (the 8-bit view's gray), the highlight test, gray_level and gray_f32 (the fft input's planes) -- on every pixel of a
// buffer allocated at its exact size, at the byte offset the caller asks for (an odd one: a padded row), so that a build with
// -fsanitize=address,undefined (tests/test_framepx16_hostcheck.py) turns a read outside the buffer or a misaligned access into a
// failure.  Usage: framepx16_hostcheck IN.bin OUT.bin; IN = C, red_index, byte offset, n (int32), then offset + n * C * 2 bytes;
// OUT = per pixel g16, gray8, highlight, level (int32) and the bits of the float32 gray (uint32).
#include "../../360cam-pgm-3dgs-tools_amd/csrc/gs360_framepx.h"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace gs360;

template <int C>
static void run(const uint8_t* px, int n, int red, std::vector<uint32_t>& out) {
    for (int k = 0; k < n; ++k) {
        const uint8_t* p = px + (size_t)k * C * 2;
        const int g16 = gray_of<C, uint16_t>(p, red);
        const float f = gray_f32<C, uint16_t>(p, red);
        uint32_t bits;
        std::memcpy(&bits, &f, 4);
        out.push_back((uint32_t)g16);
        out.push_back((uint32_t)gray8_of<C, uint16_t>(p, red));
        out.push_back((uint32_t)(g16 >= kFs16Highlight));
        out.push_back((uint32_t)gray_level<C, uint16_t>(p, red));
        out.push_back(bits);
    }
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[4];
    if (fread(head, 4, 4, f) != 4) return 3;
    const int C = head[0], red = head[1], off = head[2], n = head[3];
    if (off < 0 || n < 1 || (C != 1 && C != 3 && C != 4) || (red != 0 && red != 2)) return 3;
    std::vector<uint8_t> buf((size_t)off + (size_t)n * C * 2);
    if (fread(buf.data(), 1, buf.size(), f) != buf.size()) return 3;
    fclose(f);
    std::vector<uint32_t> out;
    if (C == 1) run<1>(buf.data() + off, n, red, out);
    else if (C == 3) run<3>(buf.data() + off, n, red, out);
    else run<4>(buf.data() + off, n, red, out);
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) return 4;
    fclose(f);
    return 0;
}
