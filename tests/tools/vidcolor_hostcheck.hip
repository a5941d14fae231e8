// vidcolor_hostcheck.hip -- steps VID-COLOR v1's per-lane functions (csrc/gs360_vidsteps.h) on the host, one call per pixel group as
// the kernel's lanes make them, with every plane and the destination allocated at its exact size ((H - 1) * stride + one row), so that
// AddressSanitizer sees any byte read or written outside them.  tests/test_vidcolor_hostcheck.py builds and feeds it.
//   in.bin : 12 int32 (depth, W, H, sx, sy, y stride, cb stride, cr stride, dst stride, 0, 0, 0), 8 int32 coefficients (VcCoef),
//            9 + 16384 + 2048 float32 (primaries, linear, encode), then the three planes laid out with their strides
//   out.bin: the destination, laid out with its stride, 0xA5 where nothing was written
#include "../../360cam-pgm-3dgs-tools_amd/csrc/gs360_vidsteps.h"
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
    std::vector<float> m(9), lin(kVcLevels), enc(2 * kVcEnc);
    bool ok = fread(head, sizeof(head), 1, f) == 1 && fread(&K, sizeof(K), 1, f) == 1 && fread(m.data(), 4, 9, f) == 9 &&
              fread(lin.data(), 4, lin.size(), f) == lin.size() && fread(enc.data(), 4, enc.size(), f) == enc.size();
    if (!ok) return 3;
    const int depth = head[0], bytes = depth == 8 ? 1 : 2;
    VcImage I{};
    I.W = head[1]; I.H = head[2]; I.sx = head[3]; I.sy = head[4];
    I.ys = head[5]; I.cbs = head[6]; I.crs = head[7]; I.ds = head[8];
    const int cw = (I.W + I.sx) >> I.sx, ch = (I.H + I.sy) >> I.sy;
    const size_t ny = exact(I.H, I.ys, (size_t)I.W * bytes), ncb = exact(ch, I.cbs, (size_t)cw * bytes);
    const size_t ncr = exact(ch, I.crs, (size_t)cw * bytes), nd = exact(I.H, I.ds, (size_t)I.W * 3 * bytes);
    // malloc'ed (not vector) so that each block ends exactly where the plane ends
    uint8_t* py = (uint8_t*)malloc(ny); uint8_t* pcb = (uint8_t*)malloc(ncb); uint8_t* pcr = (uint8_t*)malloc(ncr);
    uint8_t* pd = (uint8_t*)malloc(nd);
    ok = py && pcb && pcr && pd && fread(py, 1, ny, f) == ny && fread(pcb, 1, ncb, f) == ncb && fread(pcr, 1, ncr, f) == ncr;
    fclose(f);
    if (!ok) return 3;
    memset(pd, 0xA5, nd);
    I.y = py; I.cb = pcb; I.cr = pcr; I.dst = pd;
    I.fast = (((uintptr_t)py | (uintptr_t)pcb | (uintptr_t)pcr | (uintptr_t)pd | (uint64_t)I.ys | (uint64_t)I.cbs | (uint64_t)I.crs |
               (uint64_t)I.ds) & 3u) == 0;
    I.gpr = (I.W + kVcGroup - 1) / kVcGroup;
    VcTables T;
    T.lin = lin.data();
    T.enc = reinterpret_cast<const float2*>(enc.data());
    memcpy(T.m, m.data(), sizeof(T.m));
    T.outmax = depth == 8 ? 255 : 65535;
    // whole tiles of 512 lanes, as the kernel launches them: lanes past the last group do nothing
    const uint32_t groups = vc_groups(I), lanes = (groups + 511u) / 512u * 512u;
    for (uint32_t g = 0; g < lanes; ++g) {
        if (g >= groups) continue;
        if (depth == 8) vc_group<uint8_t>(I, K, T, g);
        else vc_group<uint16_t>(I, K, T, g);
    }
    f = fopen(argv[2], "wb");
    ok = f && fwrite(pd, 1, nd, f) == nd;
    if (f) fclose(f);
    printf("%d %u\n", I.fast, groups);
    free(py); free(pcb); free(pcr); free(pd);
    return ok ? 0 : 4;
}
