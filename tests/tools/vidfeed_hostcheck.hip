// vidfeed_hostcheck.hip -- steps VID-FEED v1's (10, 8) instantiation of the per-lane functions (csrc/gs360_vidsteps.h,
// vc_group<uint16_t, uint8_t>) on the host, one call per pixel group as the kernel's lanes make them, with every plane and the
// destination allocated at its exact size ((H - 1) * stride + one row), so that AddressSanitizer sees any byte read or written outside
// them.  One run takes many cases; tests/test_vidfeed_hostcheck.py builds and feeds it.
//   in.bin : int32 n_cases, 9 + 16384 float32 (primaries, linear), 2048 float32 (encode for sRGB, outmax 255), 2048 float32 (encode
//            for the Rec.709 curve), then per case 12 int32 (W, H, sx, sy, y stride, cb stride, cr stride, dst stride, bytes the luma
//            plane's pointer is moved off its allocation's start, keep_rec709, 0, 0), 8 int32 coefficients (VcCoef) and the three
//            uint16 planes laid out with their strides
//   out.bin: per case int32 fast, int32 groups, then the uint8 destination laid out with its stride, 0xA5 where nothing was written
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
    FILE* o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    int32_t n_cases = 0;
    std::vector<float> m(9), lin(kVcLevels), enc[2] = {std::vector<float>(2 * kVcEnc), std::vector<float>(2 * kVcEnc)};
    bool ok = fread(&n_cases, 4, 1, f) == 1 && fread(m.data(), 4, 9, f) == 9 && fread(lin.data(), 4, lin.size(), f) == lin.size() &&
              fread(enc[0].data(), 4, enc[0].size(), f) == enc[0].size() && fread(enc[1].data(), 4, enc[1].size(), f) == enc[1].size();
    if (!ok) return 3;
    for (int k = 0; k < n_cases; ++k) {
        int32_t head[12];
        VcCoef K;
        if (fread(head, sizeof(head), 1, f) != 1 || fread(&K, sizeof(K), 1, f) != 1) return 3;
        VcImage I{};
        I.W = head[0]; I.H = head[1]; I.sx = head[2]; I.sy = head[3];
        I.ys = head[4]; I.cbs = head[5]; I.crs = head[6]; I.ds = head[7];
        const size_t off = (size_t)head[8];
        const int keep = head[9];
        if (I.W < 1 || I.H < 1 || (off & 1) || off > 2 || (keep & ~1)) return 3;
        const int cw = (I.W + I.sx) >> I.sx, ch = (I.H + I.sy) >> I.sy;
        const size_t ny = exact(I.H, I.ys, (size_t)I.W * 2), ncb = exact(ch, I.cbs, (size_t)cw * 2);
        const size_t ncr = exact(ch, I.crs, (size_t)cw * 2), nd = exact(I.H, I.ds, (size_t)I.W * 3);
        // malloc'ed (not vector) so that each block ends exactly where the plane ends
        uint8_t* py = (uint8_t*)malloc(ny + off); uint8_t* pcb = (uint8_t*)malloc(ncb); uint8_t* pcr = (uint8_t*)malloc(ncr);
        uint8_t* pd = (uint8_t*)malloc(nd);
        ok = py && pcb && pcr && pd && fread(py + off, 1, ny, f) == ny && fread(pcb, 1, ncb, f) == ncb && fread(pcr, 1, ncr, f) == ncr;
        if (!ok) return 3;
        memset(pd, 0xA5, nd);
        I.y = py + off; I.cb = pcb; I.cr = pcr; I.dst = pd;
        I.fast = (((uintptr_t)I.y | (uintptr_t)pcb | (uintptr_t)pcr | (uintptr_t)pd | (uint64_t)I.ys | (uint64_t)I.cbs | (uint64_t)I.crs |
                   (uint64_t)I.ds) & 3u) == 0;
        I.gpr = (I.W + kVcGroup - 1) / kVcGroup;
        VcTables T;
        T.lin = lin.data();
        T.enc = reinterpret_cast<const float2*>(enc[keep].data());
        memcpy(T.m, m.data(), sizeof(T.m));
        T.outmax = 255;
        // whole tiles of 512 lanes, as the kernel launches them: lanes past the last group do nothing
        const uint32_t groups = vc_groups(I), lanes = (groups + 511u) / 512u * 512u;
        for (uint32_t g = 0; g < lanes; ++g) {
            if (g >= groups) continue;
            vc_group<uint16_t, uint8_t>(I, K, T, g);
        }
        const int32_t tail[2] = {I.fast, (int32_t)groups};
        if (fwrite(tail, sizeof(tail), 1, o) != 1 || fwrite(pd, 1, nd, o) != nd) return 4;
        free(py); free(pcb); free(pcr); free(pd);
    }
    fclose(f);
    return fclose(o) == 0 ? 0 : 4;
}
