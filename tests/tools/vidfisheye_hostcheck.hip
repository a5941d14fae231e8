// vidfisheye_hostcheck.hip -- steps VID-FISHEYE v1's per-lane functions (csrc/gs360_vidfishsteps.h) on the host, one call per output
// pixel in the kernel's tile order, with every plane and the destination allocated at its exact size ((rows - 1) * stride + one row),
// so that AddressSanitizer sees any byte read or written outside them.  tests/test_vidfisheye_hostcheck.py builds and feeds it.
//   in.bin : 12 int32 (depth, W, H, sx, sy, y stride, cb stride, cr stride, dst stride, S, projection, 0), 8 int32 coefficients
//            (VcCoef), 10 float32 (VfView's tx .. oy16), 9 + 16384 + 2048 float32 (primaries, linear, encode), then the three planes
//            laid out with their strides
//   out.bin: the destination, laid out with its stride, 0xA5 where nothing was written
#include "../../360cam-pgm-3dgs-tools_amd/csrc/gs360_vidfishsteps.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace gs360;

static size_t exact(int rows, int64_t stride, size_t row_bytes) { return (size_t)(rows - 1) * (size_t)stride + row_bytes; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[12];
    VcCoef K;
    float vf[10];
    std::vector<float> m(9), lin(kVcLevels), enc(2 * kVcEnc);
    bool ok = fread(head, sizeof(head), 1, f) == 1 && fread(&K, sizeof(K), 1, f) == 1 && fread(vf, sizeof(vf), 1, f) == 1 &&
              fread(m.data(), 4, 9, f) == 9 && fread(lin.data(), 4, lin.size(), f) == lin.size() &&
              fread(enc.data(), 4, enc.size(), f) == enc.size();
    if (!ok) return 3;
    const int depth = head[0], bytes = depth == 8 ? 1 : 2;
    VcImage I{};
    I.W = head[1]; I.H = head[2]; I.sx = head[3]; I.sy = head[4];
    I.ys = head[5]; I.cbs = head[6]; I.crs = head[7]; I.ds = head[8];
    VfView V{};
    V.S = head[9]; V.proj = head[10];
    V.tx = vf[0]; V.ty = vf[1]; V.kx32 = vf[2]; V.ky32 = vf[3]; V.kx16 = vf[4]; V.ky16 = vf[5];
    V.ox32 = vf[6]; V.oy32 = vf[7]; V.ox16 = vf[8]; V.oy16 = vf[9];
    const int cw = (I.W + I.sx) >> I.sx, ch = (I.H + I.sy) >> I.sy;
    const size_t ny = exact(I.H, I.ys, (size_t)I.W * bytes), ncb = exact(ch, I.cbs, (size_t)cw * bytes);
    const size_t ncr = exact(ch, I.crs, (size_t)cw * bytes), nd = exact(V.S, I.ds, (size_t)V.S * 3 * bytes);
    // malloc'ed (not vector) so that each block ends exactly where the plane ends
    uint8_t* py = (uint8_t*)malloc(ny); uint8_t* pcb = (uint8_t*)malloc(ncb); uint8_t* pcr = (uint8_t*)malloc(ncr);
    uint8_t* pd = (uint8_t*)malloc(nd);
    ok = py && pcb && pcr && pd && fread(py, 1, ny, f) == ny && fread(pcb, 1, ncb, f) == ncb && fread(pcr, 1, ncr, f) == ncr;
    fclose(f);
    if (!ok) return 3;
    memset(pd, 0xA5, nd);
    I.y = py; I.cb = pcb; I.cr = pcr; I.dst = pd;
    I.fast = (((uintptr_t)py | (uintptr_t)pcb | (uintptr_t)pcr | (uint64_t)I.ys | (uint64_t)I.cbs | (uint64_t)I.crs) & 3u) == 0;
    VcTables T;
    T.lin = lin.data();
    T.enc = reinterpret_cast<const float2*>(enc.data());
    memcpy(T.m, m.data(), sizeof(T.m));
    T.outmax = depth == 8 ? 255 : 65535;
    int16_t wtab[4 * kVfPhases];
    for (int p = 0; p < kVfPhases; ++p) vf_weights(p, wtab + 4 * p);
    // whole tiles, as the kernel walks them: lanes past the view do nothing
    const int tiles_x = (V.S + kVfTileW - 1) / kVfTileW, tiles_y = (V.S + kVfTileH - 1) / kVfTileH;
    unsigned pixels = 0;
    for (int t = 0; t < tiles_x * tiles_y; ++t)
        for (int l = 0; l < kVfTileW * kVfTileH; ++l) {
            const int i = (t % tiles_x) * kVfTileW + l % kVfTileW, j = (t / tiles_x) * kVfTileH + l / kVfTileW;
            if (i >= V.S || j >= V.S) continue;
            if (depth == 8) vf_pixel<uint8_t>(I, V, K, T, wtab, i, j);
            else vf_pixel<uint16_t>(I, V, K, T, wtab, i, j);
            ++pixels;
        }
    f = fopen(argv[2], "wb");
    ok = f && fwrite(pd, 1, nd, f) == nd;
    if (f) fclose(f);
    printf("%d %u\n", I.fast, pixels);
    free(py); free(pcb); free(pcr); free(pd);
    return ok ? 0 : 4;
}
