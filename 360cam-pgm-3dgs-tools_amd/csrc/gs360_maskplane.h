// gs360_maskplane.h -- what the mask kernels (gs360_maskmorph.hip, gs360_maskshadow.hip, gs360_maskinpaint.hip), their glue
// (gs360_capi_mask.hip) and the host checks (tests/tools/mask*_hostcheck.hip) share: the jobs and launches of the families, the steps on a
// bit plane and the launch geometry of every step (MSK-SPEC v1, MSK-SHADOW v1 and MSK-INPAINT v1).  A mask lives as a bit plane: bit x & 31 of dword
// x >> 5, pw = ceil(W / 32) dwords per row, bits at columns >= W zero.  What is marked MK_HD is host-callable, so that the host
// checks can step it under a sanitizer and the glue sizes a grid with the function that bounds the kernel.
#pragma once
#include "gs360_framepx.h"

namespace gs360 {

#define MK_HD __host__ __device__

// Segmentation-mask finishing (gs360_maskmorph.hip): one step of the chain over a batch of up to GS360_MAX_VIEWS masks.  The glue
// fills the fields a step reads and gives a job that skips the step no tiles.
constexpr int kMkThreads = 256;
constexpr int kMkTileW = 32, kMkTileR = 32;              // a morph tile: output dwords x output rows
constexpr int kMkMaxElem = 1025;                         // largest element side (p = 512)
constexpr int kMkMaxHalo = kMkMaxElem / 2 / 32 + 2;      // staged dwords left and right of a tile: reach / 32 + 2
constexpr int kMkStageW = kMkTileW + 2 * kMkMaxHalo, kMkStageRows = 96;   // the LDS band: 96 rows of at most 68 dwords
constexpr int kMkFinishRows = 32;                        // rows of a workgroup of the counting pass
constexpr int kMkCompIn = 1, kMkCompOut = 2;             // morph flags: complement the plane read / written, inside the image
struct MkJob {
    const uint8_t *src, *add, *img;      // raw mask (null: all clear), manual add layer (null: none), H x W x 3 image (compose kinds)
    uint8_t* dst;
    int64_t src_stride, add_stride, img_stride, dst_stride;
    const uint32_t* in;                  // the plane a step reads ...
    uint32_t* out;                       // ... and writes (pack, finish: the one plane they work on)
    const int32_t* spans;                // morph: kh x (j1, j2), device memory
    int32_t H, W, pw, thresh;
    int32_t kh, ax, ay, halo;            // morph: element rows, anchor, staged halo dwords (mk_element_halo)
    int32_t f, s, kind, invert;          // edge fuse: strip width and vertical spread of the side seeds; output kind and polarity
    int32_t tile_base, tiles_x, flags, pad;
};
struct MkLaunch {
    MkJob job[GS360_MAX_VIEWS];
    int32_t n_jobs, total_tiles, phase, pad;
    uint32_t* counts;                    // n_jobs: set pixels of the finished masks (the caller's buffer)
};
static_assert(sizeof(MkLaunch) <= 4096, "a launch travels by value as the kernels' argument");
hipError_t launch_mask_pack_bits(const MkLaunch& L, hipStream_t s);   // mk_pack_kernel
hipError_t launch_mask_morph(const MkLaunch& L, hipStream_t s);       // mk_morph_kernel: one dilate or erode
hipError_t launch_mask_fuse(const MkLaunch& L, hipStream_t s);        // mk_fuse_kernel, phase 0 (copy) or 1 (the strips' fills)
hipError_t launch_mask_finish(const MkLaunch& L, hipStream_t s);      // mk_finish_kernel, phase 0 (add layer, count) or 1 (output)

// The shadow estimate in front of the finishing chain (gs360_maskshadow.hip): one step over a batch of up to GS360_MAX_VIEWS images.
// The gray plane has 32 pw bytes per row, the float plane of the row pass W floats (the labels take its place later), `area` one
// dword per pixel (root flags, then doubled areas).
constexpr int kMsThreads = kMkThreads;
constexpr int kMsOut = 8;                                // neighbouring outputs of one lane of the two blur passes
constexpr int kMsMaxR = 255;                             // largest filter radius
constexpr int kMsRowSeg = kMsThreads * kMsOut;           // outputs of a workgroup of the row pass
constexpr int kMsColW = 64, kMsColRows = 128;            // a column-pass tile: a wave's 64 columns x 4 waves' 32 rows
constexpr int kMsAreaRows = 16, kMsSelectRows = 8;       // cell rows of an area lane, rows of a select workgroup
constexpr int kMsComplement = 1;                         // label flag: the plane's complement (inside the image) is labelled
struct MsJob {
    const uint8_t* img;                  // H x W x 3
    uint8_t *gray, *dst;                 // gray plane; M as H x W bytes of 0 / 255
    float* mid;                          // the row pass's result
    int32_t* lab;                        // labels: a set pixel's root index y W + x, -1 elsewhere
    uint32_t* area;
    const float* k;                      // r + 1 weights, centre outward (device memory)
    const int32_t* sdiv;                 // 256 saturation divisors (device memory)
    const uint32_t *a, *b, *c;           // the planes a step reads ...
    uint32_t *out, *out2;                // ... and writes
    int64_t img_stride, dst_stride;
    int32_t H, W, pw, r;
    float t, delta_min;
    int32_t sat_max;
    uint32_t th2;                        // 2 max(1, min_area)
    int32_t tile_base, tiles_x, flags, pad;
};
struct MsLaunch {
    MsJob job[GS360_MAX_VIEWS];
    int32_t n_jobs, total_tiles, conn, pad;              // conn: 4 or 8 (label merge)
    uint32_t* counts;                    // n_jobs: set pixels of M
    uint32_t* err;                       // one word: set when a label walk ran past its bound
};
static_assert(sizeof(MsLaunch) <= 4096, "a launch travels by value as the kernels' argument");
enum MsStep { kMsPixel, kMsBlurRows, kMsBlurCols, kMsLogic, kMsLabelInit, kMsLabelMerge, kMsLabelFlatten, kMsBorder, kMsFill, kMsArea, kMsSelect };
hipError_t launch_mask_shadow(MsStep step, const MsLaunch& L, hipStream_t s);

// Inpainting the masked region (gs360_maskinpaint.hip, MSK-INPAINT v1): one step over a batch of up to GS360_MAX_VIEWS images whose
// pixels are numbered through the batch (px_base + y W + x, below 2^32).  A job's planes hold one entry per pixel: `vert` the
// distance to the nearest pixel outside F in the pixel's column (kMiFar: none within kMiMaxLevel), `lev` L and `dist` T.
constexpr int kMiThreads = kMkThreads;
constexpr int kMiMaxLevel = 4095;                        // the largest K; a level of kMiFar marks a pixel beyond it
constexpr int kMiFar = kMiMaxLevel + 1;
constexpr int kMiMaxRadius = 8, kMiMaxOffsets = 196;     // the lattice points of a disc of radius 8 without its centre
constexpr int kMiScanPer = (kMiFar + kMiThreads) / kMiThreads;   // levels a lane of the scan sums: 17, 256 x 17 >= 4097
struct MiHead {                                          // the start of the call's scratch: err cleared per call, the rest per batch
    uint32_t err, pad[15];                               // set when a lane left a bound (a defect)
    uint32_t filled[GS360_MAX_VIEWS];                    // pixels of F per job
    uint32_t hist[kMiFar + 1];                           // pixels per level over the batch; [0] stays 0
    uint32_t offs[kMiFar + 1];                           // where a level's pixels begin in the list
    uint32_t cursor[kMiFar + 1];                         // pixels of a level scattered so far
};
struct MiJob {
    uint8_t* img;                        // H x W x 3, filled in place
    const uint8_t* fill;                 // F: H x W bytes, set where > 0
    int64_t img_stride, fill_stride;
    uint16_t *vert, *lev;
    float* dist;
    const int32_t* off;                  // n_off x (dy, dx), row-major order (device memory)
    const float *rlen, *inv2;            // |r| and 1 / |r|^2 per offset (device memory)
    int32_t H, W, n_off;
    uint32_t px_base;
    int32_t tile_base, tiles_x, pad[2];
};
struct MiLaunch {
    MiJob job[GS360_MAX_VIEWS];
    int32_t n_jobs, total_tiles, level, pad;
    uint32_t items, list_cap;            // fill: the level's pixels; the list's entries
    MiHead* head;
    uint32_t* list;                      // the batch's pixels of F grouped by level
    uint32_t* levels;                    // n_jobs: K per job (the caller's buffer)
};
static_assert(sizeof(MiLaunch) <= 4096, "a launch travels by value as the kernels' argument");
enum MiStep { kMiCols, kMiRows, kMiScan, kMiScatter, kMiFill };
hipError_t launch_mask_inpaint(MiStep step, const MiLaunch& L, hipStream_t s);

// ---- bits --------------------------------------------------------------------------------------------------------------------------
MK_HD inline int mk_lo(int a, int b) { return a < b ? a : b; }
MK_HD inline int mk_hi(int a, int b) { return a > b ? a : b; }
MK_HD inline int mk_ctz(uint32_t v) { return __builtin_ctz(v); }
MK_HD inline int mk_clz(uint32_t v) { return __builtin_clz(v); }
MK_HD inline int mk_popc(uint32_t v) { return __builtin_popcount(v); }
MK_HD inline uint32_t mk_colmask(int W, int w) {         // the columns of dword w that lie inside the image
    const int left = W - 32 * w;
    return left >= 32 ? 0xffffffffu : left <= 0 ? 0u : (0xffffffffu >> (32 - left));
}
// pixel (y, x) of a plane; the four columns from x (a multiple of 4) on, clear past the row's last dword
MK_HD inline bool mk_bit(const uint32_t* plane, int pw, int y, int x) { return (plane[(int64_t)y * pw + (x >> 5)] >> (x & 31)) & 1u; }
MK_HD inline uint32_t mk_plane_nibble(const uint32_t* plane, int pw, int y, int x) {
    return (x >> 5) < pw ? (plane[(int64_t)y * pw + (x >> 5)] >> (x & 31)) & 15u : 0u;
}
// the group of four bytes at p, columns x .. x + 3 of a row of W (x < W), byte k in bits 8 k ..: one dword access where the group is
// aligned and inside the row, byte by byte otherwise.  Columns >= W load as zero and are not stored.
MK_HD inline uint32_t mk_load4(const uint8_t* p, int x, int W) {
    uint32_t v = 0;
    if (x + 4 <= W && ((uintptr_t)p & 3) == 0) __builtin_memcpy(&v, __builtin_assume_aligned(p, 4), 4);
    else
        for (int k = 0; k < 4 && x + k < W; ++k) v |= (uint32_t)p[k] << (8 * k);
    return v;
}
MK_HD inline void mk_store4(uint8_t* p, int x, int W, uint32_t v) {
    if (x + 4 <= W && ((uintptr_t)p & 3) == 0) __builtin_memcpy(__builtin_assume_aligned(p, 4), &v, 4);
    else
        for (int k = 0; k < 4 && x + k < W; ++k) p[k] = (uint8_t)(v >> (8 * k));
}
// the halo dwords a morph tile stages on either side for an element (kh x half-open spans of its kw columns): reach / 32 + 2 with the
// largest |column offset| it reaches; 0 without an element, -1 for a span outside the element
MK_HD inline int mk_element_halo(const int32_t* rows, int kw, int kh) {
    int reach = 0;
    for (int i = 0; i < kh; ++i) {
        const int j1 = rows[2 * i], j2 = rows[2 * i + 1];
        if (j1 < 0 || j2 < j1 || j2 > kw) return -1;
        if (j2 > j1) reach = mk_hi(reach, mk_hi(abs(j1 - kw / 2), abs(j2 - 1 - kw / 2)));
    }
    return kh ? reach / 32 + 2 : 0;
}

// ---- atomics: the builtins HIP's own atomicOr, atomicAdd and atomicMin are made of, which host code may call as well -------------------
MK_HD inline void mk_atomic_or(uint32_t* p, uint32_t v) { __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
MK_HD inline void mk_atomic_add(uint32_t* p, uint32_t v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
MK_HD inline int32_t mk_atomic_min(int32_t* p, int32_t v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
MK_HD inline uint32_t mk_atomic_fetch_add(uint32_t* p, uint32_t v) { return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
MK_HD inline void mk_atomic_max(uint32_t* p, uint32_t v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
MK_HD inline int32_t mk_atomic_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- launch geometry: the kernel's bound, the glue's grid and the host checks' loops all take a step's tiles or items from here ------
// A tiled step gives a workgroup w columns (pixels; dwords of the plane for the morph) of h rows; the tiles of a job are numbered
// along x first.  An item step numbers its work along one axis, kMkThreads items per workgroup.
struct MkTile { int w, h; };
constexpr MkTile kMkPackTile = {4 * kMkThreads, 1};                  // four pixels per lane
constexpr MkTile kMkMorphTile = {kMkTileW, kMkTileR};               // dwords x rows
constexpr MkTile kMkCountTile = {4 * kMkThreads, kMkFinishRows};    // finish, phase 0
// finish, phase 1: a lane's pixels (the mask four, the compose kinds one) and the tile of a workgroup's lanes
MK_HD inline int mk_output_px(int kind) { return kind == GS360_MASK_OUT_MASK ? 4 : 1; }
MK_HD inline MkTile mk_output_tile(int kind) { return {mk_output_px(kind) * kMkThreads, 1}; }
constexpr MkTile kMsPixelTile = {4 * kMsThreads, 1};
constexpr MkTile kMsRowsTile = {kMsRowSeg, 1};
constexpr MkTile kMsColsTile = {kMsColW, kMsColRows};
constexpr MkTile kMsFillTile = {kMsThreads, 1};
constexpr MkTile kMsSelectTile = {4 * kMsThreads, kMsSelectRows};
// the tiles of a job whose rows are `extent` columns long; sets the job's tiles_x
template <class Job>
MK_HD inline int64_t mk_tiles(Job& J, int extent, MkTile t) {
    J.tiles_x = (extent + t.w - 1) / t.w;
    return (int64_t)J.tiles_x * ((J.H + t.h - 1) / t.h);
}
// a dword of the plane each: fuse phase 0, logic, the label steps
template <class Job>
MK_HD inline int64_t mk_plane_items(const Job& J) { return (int64_t)J.H * J.pw; }
// fuse phase 1, the fills: dword columns of the top strip, of the bottom strip, rows of the left strip, of the right strip
MK_HD inline int64_t mk_fuse_items(const MkJob& J) { return 2 * (int64_t)J.pw + 2 * (int64_t)J.H; }
// border: the pixels of the four border lines; area: (band of kMsAreaRows cell rows, dword column), a plane of one row has no cells
MK_HD inline int64_t ms_border_items(const MsJob& J) { return 2 * (int64_t)J.W + 2 * (int64_t)J.H; }
MK_HD inline int64_t ms_area_items(const MsJob& J) { return J.H < 2 ? 0 : (int64_t)J.pw * ((J.H - 1 + kMsAreaRows - 1) / kMsAreaRows); }
// inpaint: the column pass takes a column per item, the row pass and the scatter a pixel per lane along a row, the fill a listed pixel
// per item; the scan is one workgroup
constexpr MkTile kMiRowTile = {kMiThreads, 1};
MK_HD inline int64_t mi_cols_items(const MiJob& J) { return J.W; }
MK_HD inline int64_t mk_item_tiles(int64_t items) { return (items + kMkThreads - 1) / kMkThreads; }
// one launch of a step's kernel over the batch's tiles; a batch without tiles launches nothing
template <class Launch>
hipError_t mk_launch(void (*kernel)(Launch), const Launch& L, hipStream_t s, size_t lds = 0) {
    if (L.total_tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(kernel, dim3((unsigned)L.total_tiles), dim3(kMkThreads), lds, s, L);
    return hipGetLastError();
}

// ---- device only -------------------------------------------------------------------------------------------------------------------
// a workgroup's tile of a tiled step -> its row (of tiles) and its index along x; a lane's item of an item step
template <class Job>
__device__ __forceinline__ void mk_tile_of(const Job& J, int* ty, int* tx) {
    const int t = blockIdx.x - J.tile_base;
    *ty = t / J.tiles_x;
    *tx = t - *ty * J.tiles_x;
}
template <class Job>
__device__ __forceinline__ int64_t mk_item_of(const Job& J) { return (int64_t)(blockIdx.x - J.tile_base) * kMkThreads + threadIdx.x; }
// eight neighbouring lanes' nibbles as the dword of the plane they cover (in all eight lanes) ...
__device__ __forceinline__ uint32_t mk_gather8(uint32_t nib) {
    uint32_t v = nib << (4 * (threadIdx.x & 7));
    v |= __shfl_xor(v, 1, 64); v |= __shfl_xor(v, 2, 64); v |= __shfl_xor(v, 4, 64);
    return v;
}
// ... stored by the first of them; x: the lane's first column
__device__ __forceinline__ void mk_store_word(uint32_t* plane, int pw, int y, int x, uint32_t word) {
    if ((threadIdx.x & 7) == 0 && (x >> 5) < pw) plane[(int64_t)y * pw + (x >> 5)] = word;
}
// a wave's 64 neighbouring columns of row y, one bit per lane (x: the lane's column): the ballot as two dwords of the plane
__device__ __forceinline__ void mk_store_ballot(uint32_t* plane, int pw, int y, int x, bool bit) {
    const unsigned long long row = __ballot(bit);
    const int lane = threadIdx.x & 63;
    if ((lane & 31) == 0 && (x >> 5) < pw) plane[(int64_t)y * pw + (x >> 5)] = (uint32_t)(row >> (lane & 32));
}
// the workgroup's lanes' n added to *counter: a wave sum, one LDS word, one global atomic per workgroup (a mask has one counter: few
// atomics per mask keep it from serialising the pass).  Every lane of the workgroup calls it, once per kernel.
__device__ __forceinline__ void mk_count_tail(uint32_t n, uint32_t* counter) {
    __shared__ uint32_t wg_count;
    if (threadIdx.x == 0) wg_count = 0;
    __syncthreads();
    n = wave_sum(n);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&wg_count, n);
    __syncthreads();
    if (threadIdx.x == 0 && wg_count) atomicAdd(counter, wg_count);
}

}  // namespace gs360
