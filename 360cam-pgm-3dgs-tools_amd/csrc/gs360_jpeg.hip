// gs360_jpeg.hip -- baseline JPEG scans of 8-bit images resident on the device (JPG-SPEC v1).
//
// Reference: the image writer behind the views of cli_tools/gs360_360PerspCut.py:327-338 (ffmpeg's mjpeg encoder, `-q:v`), which the
// host path leaves to Pillow.  Everything is integer arithmetic, so the scan is pinned byte for byte (tests/jpegenc_np.py).
//
//   set-up     the quantiser tables of `quality` (IJG's scaling of Annex K.1) as reciprocals, on the launch stream
//   transform  one workgroup per strip of 8 rows x 256 columns: the rows' bytes -> LDS with dword loads; a lane per block row converts
//              its 8 pixels to Y / Cb / Cr and runs the row product, a lane per block column the column product and the quantiser;
//              the zig-zag int16 coefficients leave LDS as whole dwords, the blocks of an MCU side by side
//   entropy    one wavefront per restart interval, one lane per zig-zag coefficient: the non-zero mask is a 64-bit ballot, a lane's zero
//              run the gap to the next set bit below it, its bits (ZRLs, code, value) one word of <= 59 bits; a cross-lane prefix sum of
//              the bit lengths places the words in an LDS bit buffer, and byte stuffing runs over the packed bytes (ballot + popcount)
//   placement  size first: the entropy kernel runs once without stores for the intervals' lengths, one workgroup per image turns them
//              into offsets (exclusive scan) and the scan's length, and the same kernel runs again writing at its final offsets.
//              An image whose scan exceeds its capacity gets the length UINT64_MAX and is not written at all.
// Optimal tables ("JPG-SPEC v1, optimal tables"): between transform and size a count pass (the entropy pass's lane algorithm, adding
// each lane's symbols to an LDS histogram that is flushed once per wavefront) and a table kernel (T.81 K.2 as libjpeg runs it, one
// wavefront per image and table) give every image its own four tables; size and emit then read those in place of Annex K's.
// 4:2:0 ("JPG-SPEC v1, 4:2:0"; the writer of cli_tools/gs360_DualFisheyeDistortionCalibration.py, cv2.imwrite at DF:1826-1840): a
// colour image's transform strips are 16 rows x 256 columns, 16 MCUs of four Y blocks and one Cb and one Cr block averaged over 2 x 2
// cells; the other passes walk six blocks per MCU instead of C.
// Both transform kernels are built from the same steps (jp_stage_rows, jp_luma / jp_chroma, jp_row_product, jp_column_product,
// jp_copy_out) and the entropy and count kernels from the same block walk (JpWalk).
// No float atomics; the LDS bit buffer is filled with integer ORs and the histograms with integer adds, so nothing depends on the
// order of the work.
#include "gs360_codecsteps.h"

namespace gs360 {
namespace {

constexpr int kJpThreads = 256;
constexpr int kJpTileW = 256;                          // columns of one transform strip: 32 blocks
constexpr int kJpTileBlocks = kJpTileW / 8;
constexpr int kJpRawDw = 196;                          // dwords of one staged row: 256 * 3 bytes + 3 of alignment, rounded up

// ITU-T T.81 Annex K.1, natural order
__constant__ uint8_t kJpQBase[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// zig-zag position of natural index n
__constant__ uint8_t kJpZpos[64] = {0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53,
                                    10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// Annex K.3 as (code << 5) | length: per table 256 AC entries by (run << 4) | size, then 12 DC entries by size
constexpr int kJpHuffN = 272;
struct JpHuff { uint32_t e[2][kJpHuffN]; };
constexpr uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};
constexpr JpHuff jp_make_huff() {       // Annex C: codes in order of length, symbols in HUFFVAL order
    JpHuff h{};
    for (int t = 0; t < 2; ++t) {
        uint32_t code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < kAcBits[t][len - 1]; ++i) h.e[t][kAcVals[t][k++]] = (code++ << 5) | (uint32_t)len;
            code <<= 1;
        }
        code = 0;
        k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < kDcBits[t][len - 1]; ++i) h.e[t][256 + k++] = (code++ << 5) | (uint32_t)len;   // DC HUFFVAL is 0..11
            code <<= 1;
        }
    }
    return h;
}
constexpr JpHuff kJpHuffHost = jp_make_huff();
static_assert(kJpHuffHost.e[0][0x00] == ((0xAu << 5) | 4) && kJpHuffHost.e[0][0xF0] == ((0x7F9u << 5) | 11), "Annex K.5: EOB 1010, ZRL 11111111001");
static_assert(kJpHuffHost.e[1][0x00] == ((0x0u << 5) | 2) && kJpHuffHost.e[1][0xF0] == ((0x3FAu << 5) | 10), "Annex K.6: EOB 00, ZRL 1111111010");
__constant__ JpHuff kJpHuff = kJpHuffHost;

// ---- set-up: quantiser tables ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(128) jp_quant_kernel(JpQuant* q, int quality) {
    const int t = threadIdx.x;            // table * 64 + natural index
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int v = min(max(((int)kJpQBase[t >> 6][t & 63] * s + 50) / 100, 1), 255);
    JpQuant e;
    e.recip = (1u << 24) / (uint32_t)v + 1u;
    e.half = (uint16_t)(v >> 1);
    e.zpos = kJpZpos[t & 63];
    q[t] = e;
}

// ---- transform ------------------------------------------------------------------------------------------------------------------
// out[u] = sum_x A[u][x] * s[x], A[u][x] = round(2^14 * k(u)/2 * cos((2x+1) u pi / 16)): the rows of A are even or odd about their
// middle, so each output is four products of the sums or differences of mirrored inputs (the same integers, fewer multiplies)
__device__ __forceinline__ void jp_dct8(const int (&s)[8], int (&o)[8]) {
    constexpr int c1 = 8035, c2 = 7568, c3 = 6811, c4 = 5793, c5 = 4551, c6 = 3135, c7 = 1598;
    const int e0 = s[0] + s[7], e1 = s[1] + s[6], e2 = s[2] + s[5], e3 = s[3] + s[4];
    const int d0 = s[0] - s[7], d1 = s[1] - s[6], d2 = s[2] - s[5], d3 = s[3] - s[4];
    o[0] = c4 * e0 + c4 * e1 + c4 * e2 + c4 * e3;
    o[4] = c4 * e0 - c4 * e1 - c4 * e2 + c4 * e3;
    o[2] = c2 * e0 + c6 * e1 - c6 * e2 - c2 * e3;
    o[6] = c6 * e0 - c2 * e1 + c2 * e2 - c6 * e3;
    o[1] = c1 * d0 + c3 * d1 + c5 * d2 + c7 * d3;
    o[3] = c3 * d0 - c7 * d1 - c1 * d2 - c5 * d3;
    o[5] = c5 * d0 - c1 * d1 + c7 * d2 + c3 * d3;
    o[7] = c7 * d0 - c5 * d1 + c3 * d2 - c1 * d3;
}

// R staged rows; the strips of 4:2:0 images stage 16 (96 blocks as well: 64 Y, 16 Cb, 16 Cr)
template <int R>
struct JpLds {
    uint32_t raw[R][kJpRawDw];
    alignas(16) int16_t t1[3][8][kJpTileW];           // row products, [component][row][column]; 4:2:0: Y rows 0..7, Y rows 8..15,
                                                      // [row][Cb columns 0..127 | Cr columns 0..127]
    alignas(16) int16_t zz[3 * kJpTileBlocks][64];    // [block * C + component][zig-zag position]; 4:2:0: [MCU * 6 + block of the MCU]
    JpQuant quant[128];
};

// Step 1: R rows from image row y0 on (the last row repeats below the image), npx pixels of C bytes from column x0 -> LDS with dword
// loads.  -> the rows' byte alignments, two bits each
template <int R, int C, int N>
__device__ __forceinline__ uint32_t jp_stage_rows(JpLds<N>& S, const JpJob& J, int y0, int x0, int npx) {
    static_assert(R <= N && R <= 16, "rows of the strip, alignments in one word");
    const int tid = threadIdx.x;
    uint32_t v[R], offs = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int y = min(y0 + r, J.H - 1);
        const uintptr_t a = (uintptr_t)(J.src + (int64_t)y * J.stride + (int64_t)x0 * C);
        const uint32_t* q = (const uint32_t*)(a & ~(uintptr_t)3);
        offs |= (uint32_t)(a & 3) << (2 * r);
        const int ndw = ((int)(a & 3) + npx * C + 3) >> 2;
        v[r] = tid < ndw ? q[tid] : 0u;
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (tid < kJpRawDw) S.raw[r][tid] = v[r];
    __syncthreads();
    return offs;
}
// the staged bytes of strip row r, from its first pixel
template <int N>
__device__ __forceinline__ const uint8_t* jp_row(const JpLds<N>& S, uint32_t offs, int r) {
    return (const uint8_t*)S.raw[r] + ((offs >> (2 * r)) & 3u);
}

// JFIF's Y and (cr ? Cr : Cb) of a pixel in 16-bit fixed point, as libjpeg rounds them
__device__ __forceinline__ int jp_luma(int R, int G, int B) { return (19595 * R + 38470 * G + 7471 * B + 32768) >> 16; }
__device__ __forceinline__ int jp_chroma(int cr, int R, int G, int B) {
    const int kr = cr ? 32768 : -11059, kg = cr ? -27439 : -21709, kb = cr ? -5329 : 32768;
    return (kr * R + kg * G + kb * B + (128 << 16) + 32767) >> 16;
}

// Step 2's end: the row product of eight level-shifted samples, rounded, as one 16-byte store
__device__ __forceinline__ void jp_row_product(const int (&s)[8], int16_t* dst) {
    int o[8];
    jp_dct8(s, o);
    union { int16_t h[8]; uint4 q; } w;
#pragma unroll
    for (int u = 0; u < 8; ++u) w.h[u] = (int16_t)((o[u] + 1024) >> 11);
    *(uint4*)dst = w.q;
}

// Step 3, a lane per block column (thread tid: column tid of the plane): column product, quantiser, zig-zag scatter to the block zz
__device__ __forceinline__ void jp_column_product(const int16_t (&t1)[8][kJpTileW], const JpQuant* quant, int16_t* zz) {
    const int tid = threadIdx.x, u = tid & 7;
    int s[8], o[8];
#pragma unroll
    for (int y = 0; y < 8; ++y) s[y] = t1[y][tid];
    jp_dct8(s, o);
#pragma unroll
    for (int vv = 0; vv < 8; ++vv) {
        const int coef = (o[vv] + 65536) >> 17;
        const JpQuant e = quant[vv * 8 + u];
        const uint32_t n = (uint32_t)abs(coef) + e.half;
        const int q = (int)__umulhi(n << 8, e.recip);                              // n / Q
        zz[e.zpos] = (int16_t)(coef < 0 ? -q : q);
    }
}

// Step 4: the strip's n coefficient blocks, contiguous in the scratch from block `first` on
template <int N>
__device__ __forceinline__ void jp_copy_out(const JpLds<N>& S, const JpLaunch& L, int64_t first, int n) {
    uint32_t* dst = (uint32_t*)(L.coef + first * 64);
    const uint32_t* srcw = (const uint32_t*)&S.zz[0][0];
    for (int i = threadIdx.x; i < n * 32; i += kJpThreads) dst[i] = srcw[i];
}

// One strip of 8 rows x 256 columns, one block per component and MCU.
template <int C, int N>
__device__ __forceinline__ void jp_transform_tile(JpLds<N>& S, const JpLaunch& L, const JpJob& J, int t) {
    const int tid = threadIdx.x;
    const int by = t / J.tiles_x, tx = t - by * J.tiles_x;
    const int bx0 = tx * kJpTileBlocks, nb = min(kJpTileBlocks, J.bw - bx0);
    const int x0 = bx0 * 8, npx = min(kJpTileW, J.W - x0);
    const uint32_t offs = jp_stage_rows<8, C>(S, J, by * 8, x0, npx);
    // 2. a lane per block row: colour, level shift, row product
    {
        const int b = tid & (kJpTileBlocks - 1), y = tid >> 5;
        if (b < nb) {
            int s[C][8];
            const uint8_t* row = jp_row(S, offs, y);
#pragma unroll
            for (int x = 0; x < 8; ++x) {
                const uint8_t* p = row + min(b * 8 + x, npx - 1) * C;      // the last column repeats beside the image
                if constexpr (C == 1) {
                    s[0][x] = (int)p[0] - 128;
                } else {
                    s[0][x] = jp_luma(p[0], p[1], p[2]) - 128;
                    s[1][x] = jp_chroma(0, p[0], p[1], p[2]) - 128;
                    s[2][x] = jp_chroma(1, p[0], p[1], p[2]) - 128;
                }
            }
#pragma unroll
            for (int c = 0; c < C; ++c) jp_row_product(s[c], &S.t1[c][y][b * 8]);
        }
    }
    __syncthreads();
    if (const int b = tid >> 3; b < nb) {
#pragma unroll
        for (int c = 0; c < C; ++c) jp_column_product(S.t1[c], &S.quant[c ? 64 : 0], S.zz[b * C + c]);
    }
    __syncthreads();
    jp_copy_out(S, L, J.coef_base + (int64_t)(by * J.bw + bx0) * C, nb * C);
}

// One strip of a 4:2:0 image: 16 rows x 256 columns = 16 MCUs.  J.bw counts 16 x 16 MCUs per row.
__device__ __forceinline__ void jp_transform_tile420(JpLds<16>& S, const JpLaunch& L, const JpJob& J, int t) {
    constexpr int kMcus = kJpTileW / 16;
    const int tid = threadIdx.x;
    const int my = t / J.tiles_x, tx = t - my * J.tiles_x;
    const int m0 = tx * kMcus, nm = min(kMcus, J.bw - m0);                        // the strip's MCUs
    const int x0 = m0 * 16, npx = min(kJpTileW, J.W - x0);
    const uint32_t offs = jp_stage_rows<16, 3>(S, J, my * 16, x0, npx);
    // 2a. Y: a lane per block row of the upper and of the lower block row: colour, level shift, row product
    {
        const int b = tid & (kJpTileBlocks - 1), y = tid >> 5;
        if (b < 2 * nm) {
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const uint8_t* row = jp_row(S, offs, half * 8 + y);
                int s[8];
#pragma unroll
                for (int x = 0; x < 8; ++x) {
                    const uint8_t* p = row + min(b * 8 + x, npx - 1) * 3;          // the last column repeats beside the image
                    s[x] = jp_luma(p[0], p[1], p[2]) - 128;
                }
                jp_row_product(s, &S.t1[half][y][b * 8]);
            }
        }
    }
    // 2b. chroma: a lane per row of a Cb (threads 0..127) or Cr (128..255) block: the component at full resolution over the row's
    // 2 x 16 pixels, libjpeg's h2v2 average (bias 1 at even, 2 at odd output columns), level shift, row product
    {
        const int cr = tid >> 7, y = (tid >> 4) & 7, m = tid & (kMcus - 1);
        if (m < nm) {
            const uint8_t* r0 = jp_row(S, offs, 2 * y);
            const uint8_t* r1 = jp_row(S, offs, 2 * y + 1);
            int s[8];
#pragma unroll
            for (int x = 0; x < 8; ++x) {
                const int c0 = min(m * 16 + 2 * x, npx - 1) * 3, c1 = min(m * 16 + 2 * x + 1, npx - 1) * 3;
                const int sum = 1 + (x & 1) + jp_chroma(cr, r0[c0], r0[c0 + 1], r0[c0 + 2]) + jp_chroma(cr, r0[c1], r0[c1 + 1], r0[c1 + 2]) +
                                jp_chroma(cr, r1[c0], r1[c0 + 1], r1[c0 + 2]) + jp_chroma(cr, r1[c1], r1[c1 + 1], r1[c1 + 2]);
                s[x] = (sum >> 2) - 128;
            }
            jp_row_product(s, &S.t1[2][y][cr * (kJpTileW / 2) + m * 8]);
        }
    }
    __syncthreads();
    // 3. plane 0 and 1: Y block row 0 and 1 (block tid >> 3 of the row belongs to MCU tid >> 4); plane 2: the Cb blocks, then the Cr blocks
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int b = tid >> 3;
        const int m = c < 2 ? b >> 1 : b & (kMcus - 1);
        const int blk = m * 6 + (c < 2 ? c * 2 + (b & 1) : 4 + (b >> 4));
        if (m < nm) jp_column_product(S.t1[c], &S.quant[c == 2 ? 64 : 0], S.zz[blk]);
    }
    __syncthreads();
    jp_copy_out(S, L, J.coef_base + (int64_t)(my * J.bw + m0) * 6, nm * 6);       // MCU-major, the six blocks of an MCU side by side
}

// the workgroup's job; its quantiser tables -> LDS (visible after the tile's first barrier)
template <int N>
__device__ __forceinline__ JpJob jp_tile_job(JpLds<N>& S, const JpLaunch& L) {
    if (threadIdx.x < 128) S.quant[threadIdx.x] = L.quant[threadIdx.x];
    return L.job[job_of(L, blockIdx.x, &JpJob::tile_base)];
}

__global__ void __launch_bounds__(kJpThreads) jp_transform_kernel(const JpLaunch L) {
    __shared__ JpLds<8> S;
    const JpJob J = jp_tile_job(S, L);
    if (J.C == 3) jp_transform_tile<3>(S, L, J, blockIdx.x - J.tile_base);
    else jp_transform_tile<1>(S, L, J, blockIdx.x - J.tile_base);
}

// a batch with 4:2:0 images (L.any420): their strips, and the 8-row strips of the batch's gray images
__global__ void __launch_bounds__(kJpThreads) jp_transform420_kernel(const JpLaunch L) {
    __shared__ JpLds<16> S;
    const JpJob J = jp_tile_job(S, L);
    if (J.bpm == 6) jp_transform_tile420(S, L, J, blockIdx.x - J.tile_base);
    else jp_transform_tile<1>(S, L, J, blockIdx.x - J.tile_base);             // (every C = 3 job of such a call has bpm == 6)
}

// ---- entropy --------------------------------------------------------------------------------------------------------------------
// What a lane codes of a block (lane = zig-zag position, `raw` its coefficient, `pred` the component's previous DC): lane 0 the DC
// difference, a lane with a non-zero coefficient its value behind `run` zeros (run >> 4 ZRLs, then the symbol (run & 15) << 4 | size),
// lane 63 with a zero the EOB.  The non-zero mask is a ballot, the run the gap to the next set bit below the lane.
struct JpSym { int v, size, run, tab; };                                          // tab: the block's tables, 0 for Y, 1 for Cb and Cr
__device__ __forceinline__ JpSym jp_lane_symbol(int raw, int pred, int lane, uint64_t lower) {
    JpSym s;
    s.v = lane == 0 ? raw - pred : raw;
    s.size = 32 - __clz(abs(s.v));                                                // 0 for v == 0
    const uint64_t mask = __ballot(s.v != 0) & ~1ull;                             // non-zero AC positions
    const uint64_t below = mask & lower;
    s.run = lane - (below ? 63 - __clzll(below) : 0) - 1;                         // zeros since the previous non-zero (or the DC)
    return s;
}

// A wavefront's walk over nblk blocks in scan order, cf the lane's coefficient of the first: per block the lane's symbol.  The DC
// predictions start at 0 and return to it after every per_int blocks (a restart interval).
struct JpWalk {
    const int16_t* cf;
    int nblk, bpm, per_int, bi = 0, pos = 0, left, raw;                           // pos: the block's place in its MCU
    int pred0 = 0, pred1 = 0, pred2 = 0;
    __device__ __forceinline__ JpWalk(const int16_t* cf_, int nblk_, int bpm_, int per_int_)
        : cf(cf_), nblk(nblk_), bpm(bpm_), per_int(per_int_), left(per_int_), raw(cf_[0]) {}
    __device__ __forceinline__ bool more() const { return bi < nblk; }
    __device__ __forceinline__ JpSym next(int lane, uint64_t lower) {
        const int nxt = bi + 1 < nblk ? (int)cf[(int64_t)(bi + 1) * 64] : 0;     // the next block's load flies during this one
        const int comp = bpm == 6 ? max(pos - 3, 0) : pos;                       // one block per component, or Y Y Y Y Cb Cr
        const int dc = __shfl(raw, 0, 64);
        // (named predictors, each read and written on every path: an array, or accesses under the compare chain, which become one
        // access at an indexed member, put the walk into scratch memory)
        const int p0 = pred0, p1 = pred1, p2 = pred2;
        const int pred = comp == 0 ? p0 : (comp == 1 ? p1 : p2);
        pred0 = comp == 0 ? dc : p0;
        pred1 = comp == 1 ? dc : p1;
        pred2 = comp == 2 ? dc : p2;
        JpSym sym = jp_lane_symbol(raw, pred, lane, lower);
        sym.tab = comp ? 1 : 0;
        raw = nxt;
        ++bi;
        pos = pos + 1 == bpm ? 0 : pos + 1;
        if (--left == 0) { left = per_int; pred0 = pred1 = pred2 = 0; }
        return sym;
    }
};

// One wavefront, one restart interval.  kEmit = false counts the interval's bytes (stuffing and marker included) into int_len;
// kEmit = true writes them at the image's out + int_off.
template <bool kEmit>
__global__ void __launch_bounds__(64) jp_entropy_kernel(const JpLaunch L) {
    __shared__ uint32_t huff[2][kJpHuffN];
    __shared__ uint32_t bitbuf[64];       // MSB-first: stream byte i is bits 31-8*(i&3) .. 24-8*(i&3) of word i >> 2
    const int lane = threadIdx.x;
    const int gi = blockIdx.x;
    const int j = job_of(L, gi, &JpJob::int_base);
    const JpJob J = L.job[j];
    if (kEmit && L.lengths[j] == UINT64_MAX) return;            // the scan does not fit: nothing of it is written
    const int k = gi - J.int_base, bpm = J.bpm;
    if (L.huff) {                                                                 // the image's own tables (jp_tables_kernel)
        const uint32_t* own = L.huff + (size_t)j * 2 * kJpHuffN;
        for (int i = lane; i < 2 * kJpHuffN; i += 64) (&huff[0][0])[i] = own[i];
    } else {
        for (int i = lane; i < 2 * kJpHuffN; i += 64) (&huff[0][0])[i] = (&kJpHuff.e[0][0])[i];
    }
    bitbuf[lane] = 0;
    __syncthreads();

    const int m0 = k * L.ri, m1 = min(J.n_mcu, m0 + L.ri);
    const int nblk = (m1 - m0) * bpm;
    const int16_t* cf = L.coef + (J.coef_base + (int64_t)m0 * bpm) * 64 + lane;
    uint8_t* dst = nullptr;
    if constexpr (kEmit) dst = J.out + L.int_off[gi];
    const uint64_t lower = (1ull << lane) - 1ull;
    uint32_t carry = 0, nout = 0;         // bits waiting in bitbuf (< 8), bytes produced so far
    JpWalk walk(cf, nblk, bpm, nblk);                                             // (one interval: no reset on the way)
    while (walk.more()) {
        const JpSym sym = walk.next(lane, lower);
        const int v = sym.v, size = sym.size, run = sym.run, tab = sym.tab;
        const uint32_t vbits = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1u);
        uint64_t str = 0;
        int len = 0;
        if (lane == 0) {
            const uint32_t e = huff[tab][256 + size];
            str = ((uint64_t)(e >> 5) << size) | vbits;
            len = (int)(e & 31) + size;
        } else if (v != 0) {
            const uint32_t z = huff[tab][0xF0], e = huff[tab][((run & 15) << 4) | size];
            const int zl = (int)(z & 31), nz = run >> 4;                          // up to three ZRLs in front of the code
            if (nz > 0) { str = z >> 5; len = zl; }
            if (nz > 1) { str = (str << zl) | (z >> 5); len += zl; }
            if (nz > 2) { str = (str << zl) | (z >> 5); len += zl; }
            const int cl = (int)(e & 31) + size;
            str = (str << cl) | ((uint64_t)(e >> 5) << size) | vbits;
            len += cl;
        } else if (lane == 63) {                                                  // zeros trail: EOB
            const uint32_t e = huff[tab][0x00];
            str = e >> 5;
            len = (int)(e & 31);
        }
        const int incl = wave_scan(len, lane);
        const uint32_t total = carry + (uint32_t)__shfl(incl, 63, 64);            // <= 7 + 64 * 26 bits
        if (len) {
            const uint32_t at = carry + (uint32_t)(incl - len), w0 = at >> 5, sh = at & 31;
            const uint64_t T = str << (64 - len), U = T >> sh;
            const uint32_t a = (uint32_t)(U >> 32), b = (uint32_t)U, c = sh ? (uint32_t)((T << (64 - sh)) >> 32) : 0u;
            if (a) atomicOr(&bitbuf[w0], a);
            if (b) atomicOr(&bitbuf[w0 + 1], b);
            if (c) atomicOr(&bitbuf[w0 + 2], c);
        }
        __syncthreads();
        const uint32_t nbytes = total >> 3;                                       // whole bytes: <= 208
        for (uint32_t base = 0; base < nbytes; base += 64) {
            const uint32_t i = base + lane;
            const bool act = i < nbytes;
            const uint32_t byte = (bitbuf[(i >> 2) & 63] >> (24 - 8 * (i & 3))) & 255u;
            const bool ff = act && byte == 255u;
            const uint64_t fm = __ballot(ff);
            if constexpr (kEmit) {
                if (act) {
                    uint8_t* p = dst + nout + lane + __popcll(fm & lower);
                    p[0] = (uint8_t)byte;
                    if (ff) p[1] = 0;
                }
            }
            nout += min(64u, nbytes - base) + (uint32_t)__popcll(fm);
        }
        const uint32_t left = (bitbuf[nbytes >> 2] >> (24 - 8 * (nbytes & 3))) & 255u;   // the bits of the byte still open
        __syncthreads();
        bitbuf[lane] = lane == 0 ? left << 24 : 0u;
        __syncthreads();
        carry = total & 7;
    }
    if (carry) {                                                                  // pad with 1-bits; a 0xFF pad is stuffed like any byte
        const uint32_t byte = (bitbuf[0] >> 24) | ((1u << (8 - carry)) - 1u);
        if constexpr (kEmit) {
            if (lane == 0) {
                dst[nout] = (uint8_t)byte;
                if (byte == 255u) dst[nout + 1] = 0;
            }
        }
        nout += byte == 255u ? 2 : 1;
    }
    if (k + 1 < J.n_int) {
        if constexpr (kEmit) {
            if (lane == 0) {
                dst[nout] = 0xFF;
                dst[nout + 1] = (uint8_t)(0xD0 + (k & 7));
            }
        }
        nout += 2;
    }
    if constexpr (!kEmit) {
        if (lane == 0) L.int_len[gi] = nout;
    }
}

// ---- optimal tables: count ----------------------------------------------------------------------------------------------------------
// The symbols the entropy pass will emit, per image and table, in the layout of its code table ([2][272]: AC symbols, then DC sizes at
// 256 + size).  Each image is cut into at most L.count_waves runs of whole restart intervals; a wavefront walks one run with the lane
// algorithm of the entropy pass, adds to its LDS histogram and flushes the non-zero bins once.

__global__ void __launch_bounds__(64) jp_count_kernel(const JpLaunch L) {
    __shared__ uint32_t hist[2][kJpHuffN];
    const int lane = threadIdx.x;
    const int j = blockIdx.x / L.count_waves, w = blockIdx.x - j * L.count_waves;
    const JpJob J = L.job[j];
    const int per = (J.n_int + L.count_waves - 1) / L.count_waves;               // intervals per wavefront
    const int k0 = w * per, k1 = min(J.n_int, k0 + per);
    if (k0 >= k1) return;
    for (int i = lane; i < 2 * kJpHuffN; i += 64) (&hist[0][0])[i] = 0;
    __syncthreads();
    const int bpm = J.bpm;
    const int64_t m0 = (int64_t)k0 * L.ri, m1 = min((int64_t)J.n_mcu, (int64_t)k1 * L.ri);
    const int nblk = (int)(m1 - m0) * bpm, per_int = L.ri * bpm;                 // (ri * bpm <= 393210)
    const int16_t* cf = L.coef + (J.coef_base + m0 * bpm) * 64 + lane;
    const uint64_t lower = (1ull << lane) - 1ull;
    JpWalk walk(cf, nblk, bpm, per_int);
    while (walk.more()) {
        const JpSym sym = walk.next(lane, lower);
        if (lane == 0) {
            atomicAdd(&hist[sym.tab][256 + sym.size], 1u);
        } else if (sym.v != 0) {
            atomicAdd(&hist[sym.tab][((sym.run & 15) << 4) | sym.size], 1u);
            if (sym.run >> 4) atomicAdd(&hist[sym.tab][0xF0], (uint32_t)(sym.run >> 4));
        } else if (lane == 63) {
            atomicAdd(&hist[sym.tab][0x00], 1u);
        }
    }
    __syncthreads();
    uint32_t* g = L.hist + (size_t)j * 2 * kJpHuffN;
    for (int i = lane; i < 2 * kJpHuffN; i += 64) {
        const uint32_t n = (&hist[0][0])[i];
        if (n) atomicAdd(&g[i], n);
    }
}

// ---- optimal tables: construction ------------------------------------------------------------------------------------------------
// T.81 K.2 as libjpeg's jpeg_gen_optimal_table runs it, one wavefront per table, entry e = lane + 64 * k (257 entries: the symbols and
// the pseudo-symbol 256 with count 1, which reserves the all-ones code).  The merges, the fold of the lengths above 16 and the rank are
// the shared steps of gs360_codecsteps.h (huff_merge, huff_fold_lengths, huff_rank).  Lane 0 limits the lengths to 16 and drops the
// pseudo-symbol's code; HUFFVAL orders the symbols by unlimited length, then value (a rank every lane counts for its entries), and
// the codes follow Annex C.
// hist: per_image ? the count pass's [image][2][272] (block = image * 4 + {DC0, AC0, DC1, AC1}) : [block][256] counts.
// huff (optional): the coder's (code << 5) | length entries, [image][2][272].  tables: [block][272] = 16 BITS + HUFFVAL, zero padded.
__global__ void __launch_bounds__(64) jp_tables_kernel(const uint32_t* hist, int per_image, uint32_t* huff, uint8_t* tables) {
    __shared__ uint8_t cs[257];                   // unlimited code lengths (< 64 for counts that sum below 10^9)
    __shared__ int bits[64];
    __shared__ uint32_t word[256];                // (code << 5) | length of the symbol of HUFFVAL rank r
    __shared__ uint8_t out[kJpHuffN];
    const int lane = threadIdx.x, b = blockIdx.x;
    const int ac = b & 1;
    const uint32_t* src = per_image ? hist + (size_t)(b >> 1) * kJpHuffN + (ac ? 0 : 256) : hist + (size_t)b * 256;
    const int nsrc = per_image && !ac ? 16 : 256;
    uint32_t f[5];
    int len[5];
    bool used[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int e = lane + 64 * k;
        f[k] = e < nsrc ? src[e] : (e == 256 ? 1u : 0u);
        used[k] = f[k] != 0;
    }
    for (int i = lane; i < kJpHuffN; i += 64) out[i] = 0;
    bits[lane] = 0;
    const bool any = __ballot(used[0] || used[1] || used[2] || used[3]) != 0;     // a real symbol with a count
    huff_merge(f, used, len, lane);
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int e = lane + 64 * k;
        if (e < 257) cs[e] = (uint8_t)len[k];
        if (e < 257 && len[k]) atomicAdd(&bits[len[k] & 63], 1);
    }
    __syncthreads();
    if (lane == 0 && any) {
        // (the j > 0 and i > 0 guards never bind for counts that sum below 10^9; they keep other input from walking out of bits[])
        huff_fold_lengths(bits, 16);
        int i = 16;
        while (i > 0 && bits[i] == 0) --i;
        if (i > 0) bits[i] -= 1;                                                  // the pseudo-symbol's code
        uint32_t code = 0;
        int r = 0;
        for (int l = 1; l <= 16; ++l) {
            out[l - 1] = (uint8_t)bits[l];
            for (int n = 0; n < bits[l] && r < 256; ++n) word[r++] = (code++ << 5) | (uint32_t)l;
            code <<= 1;
        }
    }
    __syncthreads();
    uint32_t mine[4] = {0, 0, 0, 0};
    if (any) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e = lane + 64 * k, le = len[k];
            if (!le) continue;
            const int rank = huff_rank(cs, 256, le, e);
            out[16 + rank] = (uint8_t)e;
            mine[k] = word[rank];
        }
    }
    __syncthreads();
    uint8_t* dst = tables + (size_t)b * kJpHuffN;
    for (int i = lane; i < kJpHuffN; i += 64) dst[i] = out[i];
    if (huff) {
        uint32_t* h = huff + (size_t)(b >> 1) * kJpHuffN + (ac ? 0 : 256);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e = lane + 64 * k;
            if (e < nsrc) h[e] = mine[k];
        }
    }
}

// ---- placement: one workgroup per image, exclusive scan of its intervals' lengths -------------------------------------------------
__global__ void __launch_bounds__(kPlaceThreads) jp_offsets_kernel(const JpLaunch L) {
    const JpJob J = L.job[blockIdx.x];
    const unsigned long long run = place_pieces(L.int_len + J.int_base, L.int_off + J.int_base, J.n_int);
    if (threadIdx.x == 0) L.lengths[blockIdx.x] = run <= J.cap ? run : UINT64_MAX;
}

}  // namespace

hipError_t launch_jpeg_scan(const JpLaunch& L, hipStream_t s) {
    hipLaunchKernelGGL(jp_quant_kernel, dim3(1), dim3(128), 0, s, L.quant, L.quality);
    if (L.any420) hipLaunchKernelGGL(jp_transform420_kernel, dim3(L.total_tiles), dim3(kJpThreads), 0, s, L);
    else hipLaunchKernelGGL(jp_transform_kernel, dim3(L.total_tiles), dim3(kJpThreads), 0, s, L);
    if (L.huff) {                                                                 // optimal tables: zero + count, tables
        const hipError_t e = hipMemsetAsync(L.hist, 0, (size_t)L.n_jobs * 2 * kJpHuffN * sizeof(uint32_t), s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(jp_count_kernel, dim3(L.n_jobs * L.count_waves), dim3(64), 0, s, L);
        hipLaunchKernelGGL(jp_tables_kernel, dim3(L.n_jobs * 4), dim3(64), 0, s, (const uint32_t*)L.hist, 1, L.huff, L.tables);
    }
    hipLaunchKernelGGL(jp_entropy_kernel<false>, dim3(L.total_int), dim3(64), 0, s, L);
    hipLaunchKernelGGL(jp_offsets_kernel, dim3(L.n_jobs), dim3(kPlaceThreads), 0, s, L);
    hipLaunchKernelGGL(jp_entropy_kernel<true>, dim3(L.total_int), dim3(64), 0, s, L);
    return hipGetLastError();
}

hipError_t launch_jpeg_huff_tables(const uint32_t* hist, int n_tables, uint8_t* tables, hipStream_t s) {
    hipLaunchKernelGGL(jp_tables_kernel, dim3(n_tables), dim3(64), 0, s, hist, 0, (uint32_t*)nullptr, tables);
    return hipGetLastError();
}

}  // namespace gs360
