// gs360_kernels.h -- device-side parameter blocks shared by the kernels and the C-ABI glue.
// gfx950 only; no portability layer.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <mutex>
#include <vector>

#include "../../include/gs360.h"

namespace gs360 {

// Output tile of one 256-thread workgroup: 64 px wide (one wavefront = 64 consecutive pixels of a row),
// 16 rows tall (4 wavefronts x 4 rows each).
constexpr int kTileW = 64;
constexpr int kRowsPerWave = 4;
constexpr int kWaves = 4;                        // wavefronts per workgroup
constexpr int kTileH = kWaves * kRowsPerWave;
constexpr int kHalfRows = kRowsPerWave / 2;   // level views: half of a wavefront's rows are horizon mirrors

// ------------------------------------------------------------------------------------------------
// EQ-SPEC v1 per-view constants.  Host computes them in float64 and rounds once.
// ------------------------------------------------------------------------------------------------
struct EqView {
    float sxu, syv;      // tan(hfov/2)/out_w, tan(vfov/2)/out_h
    float sp, cp;        // sin / cos of pitch
    float x0f32;         // 32 * frac((yaw/360 + 1/2) * W - 1/2)
    int32_t out_w, out_h;
    int32_t tiles_x, tiles_y;
    int32_t tile_base;   // first tile index of this view's RING inside one frame
    int32_t level;       // pitch == 0 exactly (sp == 0, cp == 1): horizon-symmetric fast path
    int32_t fish;        // equidistant-fisheye output (GS360_EQ_FISHEYE_OUT): sxu/syv = fov/180/size, general row path
    int32_t blocked;     // RGB bilinear only: 1 = 4-row x 16-column gather patches instead of 64-pixel rows (strong minification);
                         // 2 = the view is rendered by eq_staged_kernel (LDS-staged source texels; all views of the launch then are)
    int32_t pad_;
    // the two per-member scalars of a yaw ring, adjacent and 8-byte aligned: the kernel reads them with one scalar load
    int32_t x0i32;       // 32 * (floor((yaw/360 + 1/2) * W - 1/2) mod W)
    int32_t flip;        // ring member whose pitch is MINUS the ring's first view's pitch: rows run bottom-up, latitude negated
};
static_assert(sizeof(EqView) == 64 && offsetof(EqView, x0i32) % 8 == 0, "EqView layout");

struct EqLaunch {
    const uint8_t* src[GS360_MAX_FRAMES];
    const uint8_t* mask[GS360_MAX_FRAMES];   // optional keep-BIT images ((H + 1) rows of mask_stride bytes, see mask_pack_kernel), all null when unused
    uint8_t* dst[GS360_MAX_FRAMES * GS360_MAX_VIEWS];
    EqView view[GS360_MAX_VIEWS];
    float kx32, ky32;    // 32*W/(2*pi), 32*H/pi
    int32_t W, H;
    int32_t y0i32;       // 16*H - 16
    int32_t n_views, n_frames;
    int32_t tiles_per_frame, total_tiles, chunk;  // chunk = ceil(total_tiles / 8) (XCD swizzle)
    const int16_t* cubic_tab;   // 32*32*16 int16 (device) when interp == cubic
    int64_t src_stride;
    int64_t mask_stride;
    int64_t dst_stride;  // 0 = tight (out_w * C)
    // Yaw rings: views [ring_first[g], ring_first[g] + ring_count[g]) share every EQ-SPEC constant except the integer
    // longitude offset x0i32 (and the sign of the pitch: `flip`), so one workgroup evaluates the coordinates of a tile once
    // and samples it for every member.  Tiles are numbered per RING (view[ring_first[g]].tile_base); the 16-bit kernel
    // runs full rings as well.
    int32_t n_rings;
    int32_t xcd_group_log2;   // >= 0: XCD x takes runs of 2^g consecutive tiles round-robin (rings of unequal size in one launch:
                              // contiguous chunks would hand whole rings to single XCDs); -1: contiguous chunks (`chunk`)
    int32_t ring_first[GS360_MAX_VIEWS];   // 32-bit on purpose: sub-dword fields of the kernel argument are fetched with VECTOR loads
    int32_t ring_count[GS360_MAX_VIEWS];   // (a memory round trip per wavefront), dwords with scalar loads
    // The cubic variants run persistent workgroups (one LDS weight table per workgroup): the caller sets `persist_blocks` (grid
    // cap, 0 = one tile per workgroup); the launcher fills `grid_total` (positions of the tile order to walk).
    int32_t persist_blocks, grid_total;
};

// ------------------------------------------------------------------------------------------------
// table-mode remap (cv2.remap semantics)
// ------------------------------------------------------------------------------------------------
struct TableLaunch {
    const uint8_t* src;
    const float* map_x;
    const float* map_y;
    const uint8_t* valid;  // may be null
    // a map plan instead of map_x / map_y / valid (map_pack_kernel; null = float maps): 5 bytes per pixel
    const uint32_t* packed;     // x + 8 (12 bits) | y + 8 (12 bits) | x phase (5 bits) | low 3 bits of the y phase
    const uint8_t* packed_hi;   // high 2 bits of the y phase | valid << 2
    int32_t use_valid;          // with a plan: apply its valid bit (the `valid` pointer of the float form)
    int32_t flat;               // row slots take spans of the flat output instead of row segments (table_remap_tile)
    uint8_t* dst;
    int32_t H, W, h, w;
    int64_t src_stride, dst_stride;
    int32_t interp;
    int32_t fill;
    uint8_t cval[4];
    const int16_t* cubic_tab;
    int32_t pipelined;   // W >= 8 and 32-bit tap offsets: split fetch/blend path allowed
    int32_t tiles_x;     // filled by the launcher (table_batch_tiling)
    int32_t tile_base;   // first tile of this job inside the batched launch
    // Lanczos-4, RGB: the 1-D phase table (32 x 8 float32, the floats the 2-D table was built from) and, per 2-D phase, the weight
    // pairs (taps 4, 5) of window rows 4 and 5 of the 2-D table as two dwords -- the block its sum fix-up patches.  With both
    // present the kernel rebuilds the other weights per pixel (same float32 product, same rounding) instead of reading 128 B of
    // the 128 KiB table; null = read the table.  (gs360_ctx_create checks the rebuilt weights against the table, all phases.)
    const float* lz_c1;
    const uint32_t* lz_cen;
};

// One launch for several remaps (e.g. the views of a dual-fisheye pair): no per-view launch tails.
struct TableBatch {
    TableLaunch job[GS360_MAX_VIEWS];
    int32_t n_jobs, total_tiles, chunk;
    int32_t persist_blocks;   // grid cap for kernels whose workgroups walk several tiles (0: one tile per workgroup); set by the caller
};

// ------------------------------------------------------------------------------------------------
// FE-SPEC v1 (fused dual-fisheye -> perspective)
// ------------------------------------------------------------------------------------------------
struct FeView {
    const uint8_t* src;
    uint8_t* dst;
    uint8_t* valid_out;  // may be null
    float sxu, syv, sp, cp, sy, cy;
    float k1, k2, k3, k4, p1, p2, tp1, tp2, b1, b2, f, cx0, cy0, wmax, hmax, cos_tmax;
    int32_t tang;
    int32_t W, H;        // sensor size
    int32_t out_w, out_h;
    int32_t tiles_x, tiles_y, tile_base;
};

struct FeCommon {          // per-launch constants of fe_views_kernel; the caller fills all but grid_total (tile_base of the views too)
    int32_t total_tiles, chunk, n_views;
    int32_t interp, mask_outside, mask_value;
    int64_t src_stride, dst_stride;
    uint8_t cval[4];
    const int16_t* cubic_tab;
    int32_t pipelined;
    int32_t grid_total;      // positions of the tile order (the persistent bicubic RGB variant walks them with stride gridDim.x)
};

struct FeBatch {           // kernel argument: all views of one launch + the common block
    FeView view[GS360_MAX_VIEWS];
    FeCommon common;
};

// ------------------------------------------------------------------------------------------------
// input colour stage (gs360_color.hip): DF:684-725 for 8-bit images
// ------------------------------------------------------------------------------------------------
struct ColorImage {        // the image of one apply call, 8- or 16-bit samples; the launch records below are the kernels' arguments
    const void* src; void* dst;
    int32_t H, W, red_index;           // red_index: memory index of the red channel (0 or 2)
    int64_t src_stride, dst_stride;     // bytes
};
struct ColorLaunch {
    ColorImage img;
    const void* rtab;       // device float3[n*n*256]: LUT pre-interpolated along red for every red level
    const float* tables;    // device: level positions R,G,B x 256, 256 output thresholds, packed bin levels
    const void* cube;       // device uint32[2^24]: the stage evaluated for every 8-bit pixel (NULL: evaluate per pixel from rtab / tables)
    int32_t lut_size, fixups;           // fixups: 1 or 2 in-bin threshold compares, 0 = binary search (color_build_bins)
};
struct Color16Launch {     // 16-bit images: everything per pixel, output thresholds in monotone pieces (gs360_color.hip)
    ColorImage img;
    const float* lut;       // device [b][g][r][3]
    const float* thr;       // device, concatenated pieces (sorted within a piece)
    const void* bins;       // device, color16_bins_bytes() (color16_build_bins); unused when n_pieces == 0
    float dmin[3], span[3];
    float start[4];         // piece lower bounds (start[0] unused)
    int32_t base[4], off[5];
    int32_t n_pieces, lut_size;         // n_pieces 0: passthrough
};
hipError_t launch_color16(const Color16Launch& L, int C, hipStream_t s);
size_t color16_bins_bytes();
void color16_build_bins(int n_pieces, const float* start, const int32_t* off, const float* thr, void* bins /* host, color16_bins_bytes() */);
size_t color_rtab_bytes(int lut_size);
size_t color_tables_floats();
int color_build_bins(const float* thresholds, uint8_t* bins);
hipError_t build_color_rtab(const float* d_lut, const float* d_pos_r, void* d_rtab, int lut_size, hipStream_t s);
size_t color_cube_bytes();
hipError_t build_color_cube(const ColorLaunch& L /* rtab, tables, lut_size, fixups */, void* d_cube, hipStream_t s);
hipError_t launch_color(const ColorLaunch& L, int C, hipStream_t s);

// kernel launchers (gs360_kernels.hip)
// keep-mask threshold + pack (gs360_equirect_views_masked_u8): byte masks -> bit images, one launch for all frames of a call
struct MaskPack {
    const uint8_t* src[GS360_MAX_FRAMES];
    uint32_t* dst[GS360_MAX_FRAMES];
    int32_t W, H, pitch_dw, n;   // pitch_dw = (W + 1 + 31) / 32 dwords per row; H + 1 rows are written
    int64_t stride;              // bytes per row of the byte masks
};
hipError_t launch_mask_pack(const MaskPack& P, hipStream_t s);
// equirect -> views: 8-bit (esize 1) or 16-bit (esize 2), bilinear or cubic; `staged`: bilinear RGB u8, every view with blocked == 2
// (LDS-staged 16x16 wavefront tiles)
hipError_t launch_equirect(const EqLaunch& L, int C, int esize, bool cubic, bool staged, hipStream_t s);
// source-major kernel (gs360_srcmajor.hip): one launch = one level yaw ring that fills its circle
struct SmTile { int32_t x0, y0, nrows, wch, eoff, nq, pad0, pad1; };   // box of a plan tile: first byte (in the period) / row, rows, 16-byte chunks per row; entries
struct SmPlan;
void sm_plan_free(SmPlan* p);
struct SmShape {                         // how a call's views fall into yaw rings of one size (filled by sm_eligible)
    int N, n_rings;                      // members per ring, rings
    int ref[GS360_MAX_VIEWS];            // ring -> view index of the member at the ring's origin
    int partner[GS360_MAX_VIEWS];        // ring -> the ring at minus its pitch (itself for a level ring)
    int qmap[GS360_MAX_VIEWS];           // ring * N + position -> view index
};
// the context's source-major plans: most recent geometries (a geometry may hold two: full- and half-height tiles); plans that were
// evicted wait in the graveyard for a moment at which the caller waits for the device anyway (hipFree synchronises it)
struct SmScratch {                       // the plan builder's device and host blocks, kept between builds (grow only)
    std::mutex mu;
    void *dev = nullptr, *host = nullptr;
    size_t dev_cap = 0, host_cap = 0;
    SmScratch() = default;
    SmScratch& operator=(const SmScratch& o) { dev = o.dev; host = o.host; dev_cap = o.dev_cap; host_cap = o.host_cap; return *this; }
};
struct SmCache {
    std::mutex mu;
    SmScratch scratch;
    std::vector<SmPlan*> plans, graveyard;
    size_t cap = 16;
    uint64_t builds = 0;                 // plans built by this context (hits build nothing: tests count instead of timing)
    uint64_t build_us = 0;               // ... and the wall time those builds took in all (coordinate kernels, copy back, ordering, upload)
    uint64_t inline_frees = 0;           // plans released inside a call because nobody synchronised for 64 evictions
};
void sm_cache_drain(SmCache& cache);     // releases the graveyard (gs360_sync, gs360_ctx_destroy)
void sm_cache_destroy(SmCache& cache);
bool sm_eligible(const EqLaunch& L, int C, int esize, int interp, bool masked, SmShape* S);
int sm_prepare(const EqLaunch& L, const SmShape& S, SmCache& cache, bool masked, int Bx, int R, int G_opt, bool adapt, int max_box_pct, size_t lds_limit, int n_cu,
               hipStream_t s, hipError_t* herr, SmPlan** out, int* box_pct);
int sm_launch(const EqLaunch& L, const SmShape& S, const SmPlan* plan, int G_opt, bool stage_regs, size_t lds_limit, int n_cu, hipStream_t s, hipError_t* herr,
              int* info /* [4]: box overhead %, tile rows, images per workgroup, 1 = the register-staging kernel */);
void sm_release(SmCache& cache, SmPlan* plan);
void build_cubic_table(int16_t* out);      // host: OpenCV initInterTab2D(INTER_CUBIC, fixpt) restated, 32*32*16
void build_lanczos4_table(int16_t* out);   // host: initInterTab2D(INTER_LANCZOS4, fixpt) restated, 32*32*64
void build_coef1d(float* out);             // host: the float32 1-D phase tables (linear, cubic, lanczos4) of the CV_16U samplers, 448
hipError_t launch_bswap16(uint16_t* buf, size_t n, hipStream_t s);            // gs360_u16.hip: in-place byte swap of 16-bit samples
hipError_t launch_arith_selftest(uint32_t seed, int blocks, int iters, unsigned long long* d_bad, hipStream_t s);
hipError_t launch_table_u16_batch(TableBatch& B, int C, const float* coef, const uint16_t cval[4], hipStream_t s);   // all jobs share interp
hipError_t launch_table(const TableLaunch& L, int C, hipStream_t s);
// map plan: float maps (+ valid) -> the packed form; `nearest` packs cvRound(map) instead of the 1/32-pixel fixed point
constexpr int kMapPlanMaxDim = 4079;     // x + 8, y + 8 of any position that still touches the image fit 12 bits
// (map plans: gs360_table.hip, map_pack_kernel) a packed position back as the floats k / 32 (or the integer position for nearest): what the samplers' own cvRound(. * 32) maps to k again
__device__ __forceinline__ void planned_coords(const uint32_t P, const uint32_t hb, const bool nearest, float& mx, float& my) {
    const int ix = (int)(P & 0xfffu) - 8, iy = (int)((P >> 12) & 0xfffu) - 8;
    if (nearest) {
        mx = (float)ix;
        my = (float)iy;
        return;
    }
    mx = (float)(ix * 32 + (int)((P >> 24) & 31u)) * 0.03125f;
    my = (float)(iy * 32 + (int)((P >> 29) | ((hb & 3u) << 3))) * 0.03125f;
}

hipError_t launch_map_pack(const float* map_x, const float* map_y, const uint8_t* valid, int64_t n, int nearest,
                           uint32_t* packed, uint8_t* packed_hi, hipStream_t s);
// LDS-staged table kernel (gs360_tablestage.hip): bilinear RGB u8 through a map plan's STAGE PLAN -- per source size the output cut into
// tiles of 64 pixels x R rows, per tile the box of source texels its taps touch, per pixel one dword (LDS offset | phases), tile-major
struct TsTile { int32_t x0b, y0, nrows, wch, magic, chunks, ty, tx; };       // box of a tile: first byte of a source row, first row, rows, 16-byte chunks
                                                                              // per row; ceil(2^20 / wch); chunks of the box; tile row / column in the output
struct TsPlan {
    int W = 0, H = 0, R = 0, h = 0, w = 0, use_valid = 0;            // key: source size, tile rows, whether the valid bit is applied
    uint8_t* d_recs = nullptr;                                        // per tile: 64-byte head (TsTile) + R x 64 plan words
    int n_tiles = 0, tiles_x = 0;
    int max_box = 0;                                                  // bytes of the largest box
    int slow_tiles = 0;                                               // tiles whose box exceeded the budget (every pixel redone from memory)
};
void ts_plan_free(TsPlan* p);
TsPlan* ts_build_plan(const uint32_t* d_packed, const uint8_t* d_hi, int h, int w, int W, int H, int R, int use_valid, int box_budget, hipStream_t s,
                      hipError_t* herr);
struct TsJobDesc {
    const uint8_t* src;
    uint8_t* dst;
    const uint32_t* packed;
    const uint8_t* packed_hi;
    const TsPlan* plan;
    int64_t src_stride, dst_stride;
    int32_t fill;
};
struct TsLaunch {
    TsJobDesc job[GS360_MAX_VIEWS];
    int32_t n_jobs, R;
    int32_t wg_per_cu;                   // 0 auto (probes)
    uint8_t cval[4];
};
hipError_t ts_launch(const TsLaunch& L, int n_cu, size_t lds_per_cu, hipStream_t s);
void table_batch_tiling(TableBatch& B);                               // tiles_x / tile_base of the jobs, total_tiles, chunk (both launchers)
hipError_t launch_table_batch(TableBatch& B, int C, hipStream_t s);   // all jobs share C and interp (job[0].interp)
// persist_blocks: grid cap of the persistent bicubic RGB variant (0: one tile per workgroup)
hipError_t launch_fisheye(FeBatch& B, int persist_blocks, int C, hipStream_t s);

// Frame sharpness statistics (gs360_framescore.hip, FS-SPEC v1 in DESIGN.md): one batch of up to GS360_MAX_FRAMES frames of one size.
struct FsLaunch {
    const uint8_t* src[GS360_MAX_FRAMES];
    float* small[GS360_MAX_FRAMES];      // 2 x small_h x small_w each (INTER_AREA plane, nearest-sample gray plane), or all null
    gs360_frame_stats* stats;            // n_frames records, cleared by the caller
    int64_t stride;
    int32_t H, W, C, red;
    int32_t depth;                       // bits per sample: 16 = uint16 in host byte order (FS-DEPTH16 v1), else 8
    int32_t y0, y1;                      // band rows [y0, y1)
    int32_t circle, highlights;          // GS360_FS_CIRCLE / GS360_FS_HIGHLIGHTS
    int32_t n_frames, strips, total, chunk;   // strips per frame, strip workgroups in all, ceil(total / 8) (XCD order)
    int32_t small_w, small_h;
    double scale_x, scale_y;             // cv2.resize's 1 / (small_w / W), 1 / (small_h / band height)
    gs360_frame_edge* edge;              // launch_frame_edge: n_frames records, cleared by the caller
};
hipError_t launch_frame_stats(FsLaunch& L, hipStream_t s);
// Frame edge score (FS-EDGE v1 in DESIGN.md): src, stride, H, W, C, red, y0, y1, n_frames and edge of L
hipError_t launch_frame_edge(FsLaunch& L, hipStream_t s);

// Frame FFT energy (gs360_framefft.hip, FS-FFT v1 in DESIGN.md): one batch of up to GS360_MAX_FRAMES fft inputs of one size.
struct FfPartial {                       // one column-pass workgroup's share of a frame's record
    double sum_hf, sum_hf_valid;
    int64_t n_valid;
};
struct FfLaunch {
    const float* small[GS360_MAX_FRAMES];   // 2 x h x w each: the INTER_AREA image, the gray at the nearest sample
    float* x[GS360_MAX_FRAMES];             // 2 x h x K each (re, im): row-pass output, K = w/2 + 1
    FfPartial* part;                        // n_frames x n_part
    gs360_frame_fft* out;                   // n_frames records
    int32_t n_frames, h, w, K, n_part;
    int32_t H, W, y0, y1;                   // frame size and band rows [y0, y1)
    int32_t circle, highlights;             // GS360_FS_CIRCLE / GS360_FS_HIGHLIGHTS
    double scale_x, scale_y;                // INTER_NEAREST's 1 / (w / W), 1 / (h / band height)
};
hipError_t launch_frame_fft(FfLaunch& L, hipStream_t s);
int frame_fft_partials(int h, int w);       // n_part: column-pass workgroups per frame

// Frame optical flow (gs360_frameflow.hip, FS-FLOW v1 in DESIGN.md).  A frame's state (level planes padded by 15, their Scharr
// derivatives, its corners) lives in one of kFlSlots resident slots of the context's scratch; a batch of <= GS360_MAX_FRAMES
// frames computes it through per-batch-entry work areas (mask, Sobel pairs, eigenvalues, candidate keys, counters).
constexpr int kFlSlots = 2 * GS360_MAX_FRAMES;
constexpr int kFlMaxPairs = 64;          // pairs per pair launch
struct FlCounters {
    int n_mask, n_cand;
    unsigned max_key;                    // order-preserving bits of the masked maximum eigenvalue
    int pad;
};
struct FlLaunch {
    const uint8_t* src[GS360_MAX_FRAMES];
    int32_t slot[GS360_MAX_FRAMES];      // resident slot of batch entry b
    int32_t n_frames;
    int64_t stride;
    int32_t H, W, C, red, circle;
    int32_t depth;                       // bits per sample, as FsLaunch's; the pass runs on the 8-bit view (sample >> 8)
    int32_t cx0, cy0, cw, ch, sw, sh;    // crop and small (level-0) size
    int32_t mode, kx, ky;                // 0 no resize, 1 INTER_AREA integer factors kx x ky, 2 general INTER_AREA
    double scale_x, scale_y;             // cv2.resize's 1 / (sw / cw), 1 / (sh / ch)
    int32_t levels;                      // pyramid levels (maxLevel + 1)
    int32_t lw[3], lh[3], pitch[3];      // level sizes; pitch = lw + 30 (padded rows: lh + 30)
    uint8_t* state;                      // kFlSlots x state_bytes
    size_t state_bytes, img_off[3], der_off[3], corner_off, ncorner_off;
    uint8_t* work;                       // GS360_MAX_FRAMES x work_bytes
    size_t work_bytes, mask_off, sob_off, eig_off, cnt_off, key_off;
    int32_t key_cap;                     // keys per work area: a power of two >= 2048 and >= the candidate count
};
struct FlPairs {
    int32_t prev[kFlMaxPairs], curr[kFlMaxPairs], out_index[kFlMaxPairs];   // resident slots; index into out / user_points
    int32_t n_pairs;
    gs360_flow_point* points;            // kFlMaxPairs x GS360_FLOW_MAX_CORNERS scratch
    gs360_flow_point* user_points;       // optional caller copy, indexed by out_index
    gs360_frame_flow* out;
};
hipError_t launch_frame_flow_frames(const FlLaunch& L, hipStream_t s);
hipError_t launch_frame_flow_pairs(const FlLaunch& L, const FlPairs& Q, hipStream_t s);

// Baseline JPEG scans (gs360_jpeg.hip, JPG-SPEC v1 in DESIGN.md): one batch of up to GS360_MAX_VIEWS images.  Scratch of the batch:
// quantised zig-zag coefficients (64 int16 per 8x8 block, the blocks of an MCU side by side), the quantiser table the set-up kernel
// derives from `quality`, and per restart interval its coded length and its offset in the image's scan.  With optimal tables
// (huff != nullptr) also per image the symbol counts and the coder's tables, both [2][272]: AC symbols, then DC sizes at 256 + size.
// An MCU holds bpm blocks: C of them, one per component, or with 4:2:0 subsampling ("JPG-SPEC v1, 4:2:0") of a C = 3 image six: four Y
// blocks of a 16 x 16 pixel MCU in raster order, then Cb, then Cr.
struct JpQuant {                         // one entry per (table, natural index)
    uint32_t recip;                      // floor(2^24 / Q) + 1: n / Q == (n * recip) >> 24 for n < 65793
    uint16_t half, zpos;                 // Q >> 1; the coefficient's zig-zag position
};
struct JpJob {
    const uint8_t* src;
    uint8_t* out;
    uint64_t cap;
    int64_t stride, coef_base;           // row stride in bytes; first block of the image in the coefficient scratch
    int32_t H, W, C, bw;                 // bw: MCUs per row (8x8 blocks per row; 16x16 MCUs with bpm == 6)
    int32_t n_mcu, n_int;                // MCUs, restart intervals
    int32_t tile_base, tiles_x;          // transform workgroups: strips of 8 rows x 256 columns (16 rows with bpm == 6)
    int32_t int_base, bpm;               // first interval of the image in int_len / int_off; blocks per MCU: C, or 6
};
struct JpLaunch {
    JpJob job[GS360_MAX_VIEWS];
    int32_t n_jobs, quality, ri, total_tiles, total_int;
    int32_t count_waves;                 // optimal tables only: wavefronts per image of the count pass
    int32_t any420, pad;                 // a job of the batch has bpm == 6: the transform kernel with 16 staged rows runs
    int16_t* coef;
    JpQuant* quant;                      // 2 x 64
    uint32_t* int_len;
    uint64_t* int_off;
    uint64_t* lengths;                   // n_jobs: the scans' lengths, UINT64_MAX where one exceeds its capacity
    uint32_t* hist;                      // optimal tables only: n_jobs x 2 x 272 symbol counts
    uint32_t* huff;                      // n_jobs x 2 x 272 (code << 5) | length; nullptr = the Annex K tables
    uint8_t* tables;                     // n_jobs x 4 x 272: 16 BITS + HUFFVAL of DC0, AC0, DC1, AC1 (the caller's buffer)
};
static_assert(sizeof(JpLaunch) <= 4096, "a launch travels by value as the kernels' argument");
hipError_t launch_jpeg_scan(const JpLaunch& L, hipStream_t s);
// n_tables x 256 symbol counts -> n_tables x 272 bytes (16 BITS + HUFFVAL, zero padded): the table kernel alone
hipError_t launch_jpeg_huff_tables(const uint32_t* hist, int n_tables, uint8_t* tables, hipStream_t s);

// PNG deflate streams (gs360_png.hip, PNG-SPEC v1 in DESIGN.md): one batch of up to GS360_MAX_VIEWS images.  Scratch of the batch: the
// filtered stream of every image (H rows of 1 + Wb bytes, each image's 256-byte aligned), and per chunk of kPnChunk filtered bytes its
// coded length, its offset in the image's stream, its two code tables and its segments' first bits.
constexpr int kPnChunk = 65536;          // filtered bytes of one dynamic-Huffman block
constexpr int kPnSegment = 512;          // bytes one lane parses: no match crosses a segment's end
constexpr int kPnThreads = kPnChunk / kPnSegment;
constexpr int kPnLitLen = 286, kPnDist = 30, kPnSyms = kPnLitLen + kPnDist;
struct PnJob {
    const uint8_t* src;
    uint8_t* out;
    uint64_t cap;
    int64_t stride, filt_base, n;        // row stride in bytes; the image's filtered stream in the scratch; its length H * (1 + Wb)
    int32_t H, Wb, bpp, swap;            // Wb: bytes of a row; swap: 1 for 16-bit samples (stored little-endian, written big-endian)
    int32_t row_base, chunk_base, n_chunks, pad;
    int32_t dist[3];                     // the candidate distances 1, bpp, 1 + Wb; 0: a repeat of an earlier one, or above 32768
    uint8_t dsym[3], dbits[3];           // their distance symbols and extra bits ...
    uint16_t dval[3];                    // ... and the extra bits' values
};
struct PnLaunch {
    PnJob job[GS360_MAX_VIEWS];
    int32_t n_jobs, total_rows, total_chunks, pad;
    uint8_t* filt;
    uint32_t* chunk_len;                 // total_chunks
    uint64_t* chunk_off;
    uint32_t* codes;                     // total_chunks x 320: (bit-reversed code << 5) | length, 286 literal/length then 30 distance symbols
    uint32_t* seg_off;                   // total_chunks x kPnThreads: a segment's first bit in its chunk's bytes
    uint64_t* lengths;                   // n_jobs: the streams' lengths, UINT64_MAX where one exceeds its capacity
    uint32_t* adler;                     // total_chunks x 2: the chunks' Adler-32 partial sums (the caller's buffer)
};
static_assert(sizeof(PnLaunch) <= 4096, "a launch travels by value as the kernels' argument");
hipError_t launch_png_deflate(const PnLaunch& L, hipStream_t s);

// The MCU grid of an image, for both codecs.  A colour image's luma is sampled hs x vs over 1 x 1 chroma: its MCU is 8 hs x 8 vs pixels
// and holds hs vs luma blocks in raster order, then Cb, then Cr (hs = vs = 1: one block per component).  A gray image's MCU is one
// block whatever its sampling factors say.
struct JpGrid { int mcu_w, mcu_h, bpm, mw, mh, hs, vs; int64_t mcus() const { return (int64_t)mw * mh; } };
// GS360_JPEG_444 / 422 / 420 / 440 / 411 (checked by the caller: the encoder takes _444 and _420) -> luma sampling 1x1 / 2x1 / 2x2 /
// 1x2 / 4x1
inline JpGrid jpeg_grid(int H, int W, int C, int subsampling) {
    const int hs = subsampling == GS360_JPEG_411 ? 4 : (subsampling == GS360_JPEG_422 || subsampling == GS360_JPEG_420) ? 2 : 1;
    const int vs = (subsampling == GS360_JPEG_440 || subsampling == GS360_JPEG_420) ? 2 : 1;
    JpGrid g;
    g.hs = C == 3 ? hs : 1;
    g.vs = C == 3 ? vs : 1;
    g.mcu_w = 8 * g.hs;
    g.mcu_h = 8 * g.vs;
    g.bpm = g.hs * g.vs > 1 ? g.hs * g.vs + 2 : C;
    g.mw = (W + g.mcu_w - 1) / g.mcu_w;
    g.mh = (H + g.mcu_h - 1) / g.mcu_h;
    return g;
}

// the job of a launch that workgroup (tile, interval) `index` belongs to: the last one whose `base` is <= index
template <class Launch, class Job>
__device__ __forceinline__ int job_of(const Launch& L, int index, int32_t Job::*base) {
    int j = 0;
    while (j + 1 < L.n_jobs && index >= L.job[j + 1].*base) ++j;
    return j;
}

// Baseline JPEG decoding (gs360_jpegdec.hip, JPD-SPEC v1 in DESIGN.md): one batch of up to GS360_MAX_VIEWS files.  A job's scratch
// (JdLayout) holds a header of three counters, per subsequence its exit state and the exclusive sum of the blocks completed before it,
// per workgroup boundary the entry state last propagated across it, the DC scan's chunk records, the blocks' DC values and, last,
// the coefficients (64 int16 per block in natural order, blocks in scan order).
constexpr int kJdSubseq = 128;           // GS360_JPEG_DEC_SUBSEQ_BYTES
constexpr int kJdWgSubs = 256;           // GS360_JPEG_DEC_WG_SUBSEQS: subsequences (lanes) per workgroup of the entropy passes
constexpr int kJdDcChunk = 1024;         // DC values one workgroup of the DC scan covers
struct JdLayout {
    size_t exits, sums, used, recs, carry, dc, coef, total;
    int64_t blocks;
    int32_t n_wg, dc_chunks;             // entropy workgroups; DC chunks of the component with the most blocks
};
inline JdLayout jd_layout_grid(const JpGrid& g, uint32_t n_sub) {
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    JdLayout l;
    l.blocks = g.mcus() * g.bpm;
    l.n_wg = (int32_t)((n_sub + kJdWgSubs - 1) / kJdWgSubs);
    l.dc_chunks = (int32_t)((g.mcus() * g.hs * g.vs + kJdDcChunk - 1) / kJdDcChunk);
    l.exits = 256;
    l.sums = l.exits + up((size_t)n_sub * 4);
    l.used = l.sums + up((size_t)n_sub * 4);
    l.recs = l.used + up((size_t)l.n_wg * 4);
    l.carry = l.recs + up((size_t)l.dc_chunks * 3 * 8);
    l.dc = l.carry + up((size_t)l.dc_chunks * 3 * 4);
    l.coef = l.dc + up((size_t)l.blocks * 4);
    l.total = l.coef + (size_t)l.blocks * 128;
    return l;
}
inline JdLayout jd_layout(int H, int W, int C, int subsampling, uint32_t n_sub) { return jd_layout_grid(jpeg_grid(H, W, C, subsampling), n_sub); }
struct JdJob {
    const uint8_t* scan;                 // the entropy-coded segment
    const uint4* seg;                    // per restart interval: start, length, first subsequence, first MCU
    const uint8_t* meta;                 // 4 x 272 Huffman table bytes, then 4 x 64 quantiser bytes (zig-zag order)
    uint8_t* scratch;
    uint8_t* out;
    int64_t stride;
    uint32_t n_seg, n_sub, scan_len;
    int32_t H, W, C, bpm, mw, mh, ri;    // bpm: blocks per MCU (1, 3, 4 or 6); MCU grid; MCUs per restart interval (0: none)
    int32_t hs, vs;                      // luma sampling: an MCU's first hs x vs blocks are Y, in raster order (JpGrid)
    int32_t wg_base, tile_base, tiles_x; // first entropy workgroup, first reconstruction tile (64 rows x 128 columns), tiles per row
    uint8_t tq[4], td[4], ta[4];         // per component: quantiser, DC table, AC table
    JdLayout lay;
};
// everything of a (checked) job but its places in the batch, wg_base and tile_base.  gray: `out` is the H x W plane of
// gs360_jpeg_decode_gray_u8, one byte per pixel
inline void jd_fill_job(JdJob& J, const gs360_jpeg_dec_job& j, bool gray = false) {
    const JpGrid g = jpeg_grid(j.H, j.W, j.C, j.subsampling);
    J.scan = (const uint8_t*)j.scan;
    J.seg = (const uint4*)j.segments;
    J.meta = j.tables;
    J.scratch = (uint8_t*)j.scratch;
    J.out = (uint8_t*)j.out;
    J.stride = (int64_t)(j.out_stride ? j.out_stride : (size_t)j.W * (gray ? 1 : j.C));
    J.n_seg = (uint32_t)j.n_segments;
    J.n_sub = j.n_subseq;
    J.scan_len = j.scan_len;
    J.H = j.H; J.W = j.W; J.C = j.C;
    J.bpm = g.bpm; J.mw = g.mw; J.mh = g.mh; J.hs = g.hs; J.vs = g.vs;
    J.ri = j.restart_interval;
    J.tiles_x = (j.W + 127) / 128;
    for (int q = 0; q < 4; ++q) { J.tq[q] = j.comp_tq[q] & 3; J.td[q] = j.comp_td[q] & 1; J.ta[q] = j.comp_ta[q] & 1; }
    J.lay = jd_layout_grid(g, j.n_subseq);
}
struct JdLaunch {
    JdJob job[GS360_MAX_VIEWS];
    int32_t n_jobs, total_wg, total_tiles, max_dc_chunks;
    uint32_t* status;                    // n_jobs
};
static_assert(sizeof(JdLaunch) <= 4096, "a launch travels by value as the kernels' argument");
hipError_t launch_jpeg_decode(const JdLaunch& L, bool gray, hipStream_t s);   // gray: jd_pixels_kernel's output mode

// The mask families (gs360_maskmorph.hip, gs360_maskshadow.hip) keep their jobs, launches and shared steps in gs360_maskplane.h.

// The point-cloud families (gs360_voxel.hip, gs360_octree.hip) keep their launches in gs360_voxel.h and gs360_octree.h and their
// shared steps in gs360_cloudsteps.h.

}  // namespace gs360
