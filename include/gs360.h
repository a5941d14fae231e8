/*
 * gs360.h -- C ABI of libgs360hip.so, the MI355X (gfx950) reprojection engine.
 *
 * This is the drop-in boundary for the 360PerspCut hot path.  The reference is pure Python and has
 * no FFI of its own; each entry point below replaces the native work the reference delegates to a
 * third-party binary/wheel at the cited call site (paths are into the reference repository):
 *
 *   gs360_equirect_views_u8      one `ffmpeg -vf v360=input=equirect:output=rectilinear:...` process per
 *                                (source, view): cli_tools/gs360_360PerspCut.py:310-314 (filter string),
 *                                :569-590 (run_one -> Popen), :830-836 (one job per view).
 *   gs360_remap_table_u8         cv2.remap(src, map_x, map_y, interp, borderMode=BORDER_CONSTANT,
 *                                borderValue=float(mask_value)) followed by `out[~valid] = mask_value`:
 *                                cli_tools/gs360_DualFisheyeDistortionCalibration.py:2001-2014 (image),
 *                                :2031-2043 (mask, INTER_NEAREST), :1198-1212 (undistort).
 *   gs360_fisheye_views_u8       the same call sites with the map of DF:1759-1823
 *                                (build_direct_perspective_map_for_lens) evaluated in-kernel instead of
 *                                being read from a table (FE-SPEC v1).
 *
 * Conventions: extern "C", plain pointers and sizes, POD structs, no exceptions across the boundary.
 * Every function returns 0 on success or a negative gs360_status; gs360_last_error() returns the
 * calling thread's last message.  The caller owns every buffer it passes in; the library never frees
 * caller memory.  One ctx per device; calls on different ctx are fully concurrent; calls on one ctx
 * are ordered per `slot` (each slot is a HIP stream) and are ASYNCHRONOUS unless stated otherwise --
 * gs360_sync(ctx, slot) waits.  Images are interleaved HWC uint8, C in {1,3,4}.
 */
#ifndef GS360_H
#define GS360_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 6): + gs360_ctx_set_option / _get_option / gs360_device_pci_bus_id (added in round 5 without a bump), the table_stage* options; the
 * library no longer reads GS360_RING, GS360_XCD_GROUP, GS360_EQ_PERSIST, GS360_TABLE_PERSIST, GS360_LANCZOS_TABLE, GS360_TABLE_ROWS from
 * the environment (context options of the same names do that: INTEGRATION.md section 2.1).  A binding checks gs360_abi_version() first.
 * Entry points added since (frame statistics, JPEG scans, gs360_jpeg_decode_u8 / gs360_jpeg_decode_gray_u8 / gs360_jpeg_decode_scratch) only add symbols and leave
 * every existing signature and struct alone, so the number stays. */
#define GS360_ABI_VERSION 2

typedef enum gs360_status {
    GS360_OK = 0,
    GS360_ERR_ARG = -1,         /* bad argument (NULL, size, channels, slot ...) */
    GS360_ERR_HIP = -2,         /* a HIP runtime call failed; text in gs360_last_error */
    GS360_ERR_NODEV = -3,       /* no usable GPU */
    GS360_ERR_UNSUPPORTED = -4, /* valid request this build does not implement */
    GS360_ERR_NOMEM = -5,
    GS360_ERR_INTERNAL = -6     /* a kernel's own bound was exceeded (a defect): the call's results are not to be used */
} gs360_status;

/* values equal cv2.INTER_NEAREST / INTER_LINEAR / INTER_CUBIC / INTER_LANCZOS4 (DF:59-64) */
#define GS360_INTERP_NEAREST 0
#define GS360_INTERP_LINEAR 1
#define GS360_INTERP_CUBIC 2
#define GS360_INTERP_LANCZOS4 4 /* table remap and fused fisheye only (8x8 taps) */

/* flags of gs360_equirect_views_u8: the views are EQUIDISTANT-FISHEYE outputs instead of rectilinear ones -- the
 * `fisheyeXY` preset's `v360=...:output=fisheye:d_fov=...` jobs (cli_tools/gs360_360PerspCut.py:351-414).  hfov_deg /
 * vfov_deg of each view are then the full horizontal / vertical field of view of the fisheye image (image-plane radius
 * <-> off-axis angle, 90 degrees at radius 1; for v360's d_fov: hfov = d_fov * w / hypot(w, h)). */
#define GS360_EQ_FISHEYE_OUT 0x1u

/* limits of one batched launch (larger requests are split internally) */
#define GS360_MAX_VIEWS 16
#define GS360_MAX_FRAMES 16

typedef struct gs360_ctx gs360_ctx;

/* One output view: the numeric fields of ViewSpec (cli_tools/gs360_360PerspCut.py:32-45). */
typedef struct gs360_view {
    double yaw_deg;   /* + = look right */
    double pitch_deg; /* + = look up */
    double hfov_deg;
    double vfov_deg;
    int32_t width;
    int32_t height;
} gs360_view;

/* SensorCalibration (cli_tools/gs360_DualFisheyeDistortionCalibration.py:67-85), numeric fields. */
typedef struct gs360_calib {
    int32_t width;
    int32_t height;
    double f, cx, cy, k1, k2, k3, k4, p1, p2, b1, b2;
} gs360_calib;

/* ---- library / device ---------------------------------------------------------------------- */
int gs360_abi_version(void);
int gs360_device_count(void);
/* copies the calling thread's last error text (NUL terminated); returns its length */
int gs360_last_error(char *buf, size_t buf_len);
/* n_slots HIP streams are created (1..16) */
int gs360_ctx_create(int device, int n_slots, gs360_ctx **out);
int gs360_ctx_destroy(gs360_ctx *ctx);
int gs360_device_info(gs360_ctx *ctx, char *name, size_t name_len, int32_t *cu_count, uint64_t *hbm_bytes);
/* "domain:bus:device.function" of the context's GPU (>= 16 bytes): lets a multi-process job prove that its ranks sit on DISTINCT
 * devices (bench.py gathers it from every rank; the reference fans jobs out over one machine's workers, PC:830-836) */
int gs360_device_pci_bus_id(gs360_ctx *ctx, char *buf, size_t buf_len);
/* Context options: kernel-selection switches for tests, probes and A/B runs (the defaults are the measured optima; results never depend
 * on them).  The reference has no counterpart (it shells out to ffmpeg / calls cv2.remap: PC:310-314, DF:2001); a binding needs them
 * only to pin a kernel variant.  gs360_ctx_create seeds the documented user switches ONCE from the environment (GS360_STAGE,
 * GS360_LANEMAP, GS360_SRCMAJOR, GS360_COLOR_CUBE, GS360_TABLE_STAGE); after that the library never reads the environment -- set options here instead.
 *   "lanemap"        -1 auto | 0 rows | 1 blocked       gather kernels' lane map
 *   "stage"          -1 auto | 0 never | 1 always       LDS-staged equirect kernel
 *   "srcmajor"       -1 auto | 0 never | 1 always       source-major equirect kernel (yaw rings of one size, level or in +/- pitch pairs:
 *                                                       the default / full360coverage / fisheyelike presets); "srcmajor_bx" (bytes per tile row,
 *                                                       multiple of 16), "srcmajor_rows" (source rows per tile), "srcmajor_images"
 *                                                       (0 auto | 1..12 dividing twice the ring size: images of a tile one workgroup walks),
 *                                                       "srcmajor_adapt" (1 | 0: calls too small to fill the GPU take tiles of half the height)
 *   "ring"           0 auto | n                         at most n views share one coordinate evaluation
 *   "xcd_group"      -2 auto | -1 chunks | g            tile order across the XCDs
 *   "eq_persist", "table_persist"                       grid caps of the persistent kernels (table_persist: -1 auto)
 *   "lanczos_table", "table_rows"                       0 | 1: A/B references of the Lanczos-4 weight rebuild and the flat spans
 *   "color_cube"     -1 / 1 tabulate | 0 per pixel      8-bit colour stage (read by gs360_color_plan_create)
 *   "table_stage"    -1 auto | 0 never | 1 always       LDS-staged table kernel (bilinear RGB through map plans; auto: plans whose tiles have boxes);
 *                                                       "table_stage_rows" (8 | 16 | 32: rows of its 64-pixel tiles), "table_stage_wgs" (0 auto | 1..4
 *                                                       workgroups per CU)
 *   "jpeg_count_waves" 1..65535 (256)                   gs360_jpeg_scan_opt_u8: wavefronts that share one image's symbol count (each walks a run of
 *                                                       whole restart intervals and flushes its histogram once; at or above the interval count:
 *                                                       one flush per interval)
 * Read-only (get): "last_eq_kernel" -- which kernel the last equirect call launched: 0 gather, 1 LDS-staged, 2 source-major, -1 none yet;
 * "last_srcmajor_box_pct" -- tile-box bytes of the last source-major plan in percent of the grid cells they stand for;
 * "last_srcmajor_rows", "last_srcmajor_images" -- tile rows and images per workgroup of the last source-major launch;
 * "srcmajor_plan_builds" -- source-major plans this context has built so far (a call on a cached geometry builds none), "srcmajor_plan_build_us"
 * -- the wall time those builds took in all, "srcmajor_plans" -- plans
 * it holds, "srcmajor_inline_frees" -- evicted plans it had to release inside a call (normally they wait for gs360_sync(ctx, -1) /
 * gs360_ctx_destroy: hipFree synchronises the device);
 * "last_table_kernel" -- jobs of the last 8-bit table call that took the LDS-staged kernel, "last_table_stage_slow_tiles" -- tiles of their
 * stage plans whose box exceeded the LDS budget.
 * Unknown keys and out-of-range values are GS360_ERR_ARG.  Thread-safe; a change applies to calls that start after it. */
int gs360_ctx_set_option(gs360_ctx *ctx, const char *key, int value);
int gs360_ctx_get_option(gs360_ctx *ctx, const char *key, int *value);

/* ---- memory (device buffers carry 64 B of readable slack after the requested size) ---------
 * Images handed to the hot-path entry points must come with that slack (the aligned 12- / 16-byte tap reads of the last
 * pixels of the last row run past the image) and, for 3-channel images, a 4-byte aligned base pointer; equirect sources
 * are at least 8 texels wide and less than 2^18 rows tall (the kernels form latitudes with 24-bit multiply-adds), H * stride < 2^32
 * and stride < 2^24 (32-bit tap offsets).  gs360_dev_alloc satisfies
 * the first two; the size limits are checked and reported as GS360_ERR_ARG / GS360_ERR_UNSUPPORTED. */
int gs360_dev_alloc(gs360_ctx *ctx, size_t bytes, void **dptr);
int gs360_dev_free(gs360_ctx *ctx, void *dptr);
int gs360_host_alloc(gs360_ctx *ctx, size_t bytes, void **hptr); /* pinned */
int gs360_host_free(gs360_ctx *ctx, void *hptr);
int gs360_upload(gs360_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes, int slot);
int gs360_download(gs360_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes, int slot);
int gs360_dev_memset(gs360_ctx *ctx, void *dst_dev, int value, size_t bytes, int slot);
/* in-place byte swap of n_samples 16-bit samples on the device (16-bit PPM frames of the video decode pipe are big-endian:
 * cli_tools/gs360_360PerspCut.py:343-347 keeps > 8-bit videos at 16 bits); asynchronous on `slot` */
int gs360_dev_bswap16(gs360_ctx *ctx, void *buf_dev, size_t n_samples, int slot);
int gs360_sync(gs360_ctx *ctx, int slot); /* slot < 0: every slot */

/* ---- timing: HIP events recorded on the slot's own stream (8 events per slot) -------------- */
int gs360_event_record(gs360_ctx *ctx, int slot, int event_idx);
int gs360_event_elapsed_ms(gs360_ctx *ctx, int slot, int event_from, int event_to, float *ms); /* syncs on event_to */
int gs360_event_sync(gs360_ctx *ctx, int slot, int event_idx);                                   /* host waits for the event */
/* work queued on waiting_slot after this call starts only when event (event_slot, event_idx) has completed: lets uploads,
 * kernels and downloads of one frame sit on DIFFERENT streams (one upload stream + one download stream is what makes
 * PCIe run full duplex: 97 GB/s against 57 GB/s with both directions on one stream, measured) */
int gs360_stream_wait_event(gs360_ctx *ctx, int waiting_slot, int event_slot, int event_idx);

/* ---- hot path: device-resident buffers, asynchronous --------------------------------------- */

/*
 * Equirectangular -> rectilinear views.  For every frame f < n_frames and view k < n_views writes
 * dst[f * n_views + k] (views[k].height x views[k].width x C, row stride dst_stride bytes, 0 = tight).
 * src_frames[f]: H x W x C equirect image, row stride src_stride bytes (0 = tight).
 * Geometry: EQ-SPEC v1: pinhole ray -> pitch about X -> yaw about Y -> lon/lat ->
 * 1/32-px fixed-point bilinear; horizontal border wraps, vertical border clamps.
 * interp: GS360_INTERP_LINEAR or GS360_INTERP_CUBIC (4x4 taps, OpenCV's fixed-point Keys A=-0.75 table; the
 * reference's own default is v360 interp=cubic, PC:730).  flags: 0 or GS360_EQ_FISHEYE_OUT.
 */
int gs360_equirect_views_u8(gs360_ctx *ctx, const void *const *src_frames, int n_frames,
                            int W, int H, int C, size_t src_stride,
                            const gs360_view *views, int n_views,
                            void *const *dst, size_t dst_stride,
                            int interp, uint32_t flags, int slot);

/*
 * Same, with a per-frame keep-mask fused into the store (BASELINE config 5; no reference counterpart): mask_frames[f]
 * is an H x W single-channel uint8 image in the SegmentationMaskTool convention (0 = masked target, 255 = keep,
 * reference cli_tools/gs360_SegmentationMaskTool.py:765-774).  The mask is sampled NEAREST at the same source
 * coordinate (texel ((sx+16)>>5 mod W, clamp((sy+16)>>5)) of EQ-SPEC v1) and the output pixel is written as 0 on all
 * channels where the mask value is < 128.  mask_stride in bytes (0 = W).
 * Only that comparison is ever used, so every call first thresholds its masks into bit images (context scratch of the slot, one
 * streaming pass over the mask bytes on the slot's stream, 6 us per 8K mask) and the kernels sample those; the masks themselves are
 * only read, and may be reused or released as soon as the call's stream work is complete.
 */
int gs360_equirect_views_masked_u8(gs360_ctx *ctx, const void *const *src_frames, const void *const *mask_frames,
                                   int n_frames, int W, int H, int C, size_t src_stride, size_t mask_stride,
                                   const gs360_view *views, int n_views,
                                   void *const *dst, size_t dst_stride,
                                   int interp, uint32_t flags, int slot);

/*
 * cv2.remap with float32 maps, BORDER_CONSTANT; then, if valid != NULL, dst[~valid] = fill_value
 * on all channels.  src: H x W x C; map_x/map_y/valid: h x w (tight); dst: h x w x C.
 * border_value: 4 doubles (cv::Scalar; Python's borderValue=float(v) is {v,0,0,0}).
 * interp: GS360_INTERP_NEAREST / LINEAR / CUBIC / LANCZOS4 (cv2's fixed-point tables for 8-bit images).
 * All pointers are device pointers.  H, W < 32767 (cv2.remap's own limit).
 */
int gs360_remap_table_u8(gs360_ctx *ctx, const void *src, int H, int W, int C, size_t src_stride,
                         const float *map_x, const float *map_y, const uint8_t *valid, int h, int w,
                         int interp, const double *border_value, int fill_value,
                         void *dst, size_t dst_stride, int slot);

/*
 * Several remaps in ONE launch (the 10 views of a dual-fisheye pair, DF:1993-2043: one cv2.remap per view): same
 * semantics per job as gs360_remap_table_u8, common channel count / interpolation / border value.  A batched launch
 * has no per-view launch tails (cfg4: -16 %).  n_jobs may exceed GS360_MAX_VIEWS (split internally).
 */
typedef struct gs360_remap_job {
    const void *src;        /* H x W x C */
    int32_t H, W;
    size_t src_stride;      /* 0 = tight */
    const float *map_x;     /* h x w */
    const float *map_y;
    const uint8_t *valid;   /* h x w or NULL */
    int32_t h, w;
    int32_t fill_value;     /* written where valid == 0 */
    void *dst;              /* h x w x C */
    size_t dst_stride;      /* 0 = tight */
} gs360_remap_job;
int gs360_remap_tables_u8(gs360_ctx *ctx, const gs360_remap_job *jobs, int n_jobs, int C, int interp,
                          const double *border_value, int slot);

/*
 * Map plans.  cv2.remap converts its float maps to 1/32-pixel fixed point on every call before it samples; the dual-fisheye
 * tool applies the SAME maps to every image pair of a run (DF:2582-2592).  A plan does the conversion once and keeps the result
 * in 5 bytes per output pixel (position, phases, valid bit) instead of two floats and a valid byte: less to read per call, no
 * conversion per pixel, identical results (integer positions are clamped to [-8, 4087], which leaves every position whose
 * Lanczos-4 window still touches a source of up to 4079 x 4079 pixels untouched; larger sources are refused with
 * GS360_ERR_UNSUPPORTED -- use the float maps).  map_x / map_y / valid are DEVICE pointers (h x w, valid may be NULL) and may be
 * released when the call returns.  `nearest` != 0 packs cvRound(map) for GS360_INTERP_NEAREST (mask cutting, DF:2031-2043);
 * a plan serves either nearest or the interpolating samplers (linear, cubic, Lanczos-4), 8- and 16-bit sources alike.
 * gs360_remap_plans_u8 = gs360_remap_tables_u8 with plans[j] in place of jobs[j].map_x / map_y (ignored); jobs[j].valid != NULL
 * asks for the plan's valid bit (fill_value where it is 0), the pointer itself is not read.
 */
typedef struct gs360_map_plan gs360_map_plan;
int gs360_map_plan_create(gs360_ctx *ctx, const float *map_x, const float *map_y, const uint8_t *valid, int h, int w,
                          int nearest, int slot, gs360_map_plan **out);
int gs360_map_plan_destroy(gs360_ctx *ctx, gs360_map_plan *plan);
int gs360_remap_plans_u8(gs360_ctx *ctx, const gs360_remap_job *jobs, const gs360_map_plan *const *plans, int n_jobs, int C,
                         int interp, const double *border_value, int slot);
/* the same on CV_16U sources (OpenCV converts the maps the same way for every depth): gs360_remap_tables_u16 with plans */
int gs360_remap_plans_u16(gs360_ctx *ctx, const gs360_remap_job *jobs, const gs360_map_plan *const *plans, int n_jobs, int C,
                          int interp, const double *border_value, int slot);

/*
 * Dual-fisheye -> perspective views with the map evaluated in-kernel (FE-SPEC v1).  View k samples
 * src_lens[k] (H x W x C of calibs[k]) with views[k].yaw_deg measured RELATIVE to that lens
 * (DF:1883).  Pixels outside the lens model / sensor get mask_value on all channels when
 * mask_outside != 0 (DF:2009-2014); border taps use {mask_value,0,0,0} as cv2 does.
 * valid_out[k] (h x w uint8, tight rows, may be NULL / may contain NULLs) receives the validity mask.
 * src_stride / dst_stride in bytes, 0 = tight; an explicit src_stride needs sensors of one width (GS360_ERR_ARG), and the views of
 * each group of GS360_MAX_VIEWS share their sensor width in any case (GS360_ERR_UNSUPPORTED) -- both refused before anything is
 * written.  A 3-channel lens image whose base is not 4-byte aligned is taken, by the byte-reading samplers (slower, same results).
 */
int gs360_fisheye_views_u8(gs360_ctx *ctx, const void *const *src_lens, const gs360_calib *calibs,
                           int C, size_t src_stride,
                           const gs360_view *views, int n_views, double lens_fov_deg,
                           int interp, int mask_outside, int mask_value,
                           void *const *dst, size_t dst_stride, uint8_t *const *valid_out, int slot);
/*
 * The same with the border taps' colour given per channel of the image AS IT LIES IN MEMORY (border_value[4], saturated to 0..255,
 * NULL = zeros), as gs360_remap_tables_u8 takes it: cv2's Scalar(mask_value,0,0,0) lands on blue of a BGR image, which is index 2
 * of an RGB(A) array.  gs360_fisheye_views_u8 = this call with {mask_value,0,0,0}.  mask_value still fills the invalid pixels.
 */
int gs360_fisheye_views_border_u8(gs360_ctx *ctx, const void *const *src_lens, const gs360_calib *calibs,
                                  int C, size_t src_stride,
                                  const gs360_view *views, int n_views, double lens_fov_deg,
                                  int interp, int mask_outside, int mask_value, const double *border_value,
                                  void *const *dst, size_t dst_stride, uint8_t *const *valid_out, int slot);

/* ---- input colour stage (dual-fisheye tool, before resampling) -------------------------------- */

/*
 * The `--input-lut` stage of cli_tools/gs360_DualFisheyeDistortionCalibration.py: apply_input_color_pipeline
 * (DF:684-725) = image_to_float01 -> apply_cube_lut_trilinear (DF:620-681) -> optional rec709_to_srgb
 * (DF:565-600) -> float01_to_image, for 8-bit images.  Because the input has 256 levels per channel and the
 * output 256, the two scalar ends of that pipeline are passed in as tables the caller computes with the reference's
 * own float32 expressions (the Python host does this with NumPy, gs360/color.py), and the kernel evaluates the
 * trilinear interpolation between them in the reference's float32 operation order:
 *   level_pos[c*256 + v]  LUT-grid position `clip((v/255 - domain_min[c]) / span[c], 0, 1) * (size-1)` of input
 *                         level v on channel c (c = 0,1,2 = R,G,B)
 *   out_thresholds[k]     k = 1..255: the smallest float32 LUT output x for which the encoded 8-bit result is >= k
 *                         (entry 0 is ignored; entries are >= 0, non-decreasing; +inf = never reached).  The encode
 *                         step is monotone, so the output level is the number of thresholds <= clip(x, 0, 1).
 *   lut                   size^3 RGB float32 triples, red fastest ([b][g][r][3], the .cube order, DF:556-562)
 * All three are HOST pointers, copied at plan creation.
 *
 * A plan evaluates the stage once for every possible 8-bit pixel (2^24 values) and keeps the results in 64 MiB of device memory;
 * gs360_color_apply_u8 then reads one table entry per pixel (GS360_ERR_NOMEM when the table cannot be allocated).  With
 * GS360_COLOR_CUBE=0 in the environment at plan creation the plan keeps its interpolation tables instead (18 MB for a 33^3 LUT)
 * and every apply evaluates the stage per pixel -- same results, about half the speed on photographs.
 */
typedef struct gs360_color_plan gs360_color_plan;
int gs360_color_plan_create(gs360_ctx *ctx, const float *lut, int lut_size, const float *level_pos,
                            const float *out_thresholds, gs360_color_plan **out);
int gs360_color_plan_destroy(gs360_ctx *ctx, gs360_color_plan *plan);
/*
 * Applies the plan to an H x W x C uint8 image (C = 3 or 4; a 4th channel is copied), device pointers, dst may equal
 * src.  red_index = 0 for RGB(A) memory order, 2 for BGR(A) (cv2.imread order, DF:697-699).
 */
int gs360_color_apply_u8(gs360_ctx *ctx, const gs360_color_plan *plan, const void *src, int H, int W, int C,
                         size_t src_stride, int red_index, void *dst, size_t dst_stride, int slot);

/* ---- 16-bit images ---------------------------------------------------------------
 * Same calls on uint16 samples (interleaved H x W x C, strides in BYTES and even).  The reference keeps 16-bit inputs at
 * native depth: cv2.imread(IMREAD_UNCHANGED) in the dual-fisheye tool (DF:735) and 16-bit PNG/TIFF stills / > 8-bit
 * videos (rgb48le) in 360PerspCut (gs360_360PerspCut.py:327-347).
 *   gs360_equirect_views_u16  EQ-SPEC v1 coordinates; bilinear (sum S a b + 512) >> 10, bicubic with the fixed-point
 *                             Keys table, exact integer sum (the value a 64-bit accumulation gives), clamped to
 *                             [0, 65535].  No fused keep-mask.
 *   gs360_remap_table_u16     cv2.remap on CV_16U: OpenCV's float-weight samplers (weights cy[k1]*cx[k2] in float32,
 *                             float32 accumulation in OpenCV's expression order, cvRound + saturate), all four
 *                             interpolations; border_value saturates to [0, 65535]; fill_value is written as uint16.
 */
int gs360_equirect_views_u16(gs360_ctx *ctx, const void *const *src_frames, int n_frames,
                             int W, int H, int C, size_t src_stride,
                             const gs360_view *views, int n_views,
                             void *const *dst, size_t dst_stride,
                             int interp, uint32_t flags, int slot);
int gs360_remap_table_u16(gs360_ctx *ctx, const void *src, int H, int W, int C, size_t src_stride,
                          const float *map_x, const float *map_y, const uint8_t *valid, int h, int w,
                          int interp, const double *border_value, int fill_value,
                          void *dst, size_t dst_stride, int slot);
/* several CV_16U remaps in one launch (the views of a dual-fisheye pair), as gs360_remap_tables_u8 */
int gs360_remap_tables_u16(gs360_ctx *ctx, const gs360_remap_job *jobs, int n_jobs, int C, int interp,
                           const double *border_value, int slot);

/*
 * The same stage for 16-bit images (DF:603-618 treat uint16 like uint8 with 65535 levels).  Nothing is tabulated on the
 * input side (float01 conversion, domain mapping and all three interpolation stages run per pixel in the reference's
 * float32 order).  Output side: n_pieces = 0 means `passthrough` = rint(clip(x) * 65535) in-kernel; otherwise the encode
 * step (Rec.709 -> sRGB through NumPy's float32 power) arrives as thresholds in n_pieces <= 4 monotone pieces of clip(x):
 * piece q covers [piece_start[q], piece_start[q+1]) (piece_start[0] is taken as 0), its thresholds are
 * thresholds[piece_off[q] .. piece_off[q+1]) (sorted), and the level is piece_base[q] + the number of them <= clip(x).
 * All pointers are HOST pointers, copied at plan creation (which also derives a 1 MiB index of the thresholds: for each of
 * 65536 equal steps of clip(x) the count up to the step and the next three thresholds, so that a pixel's level costs one
 * read per channel; the count itself stays exact).
 */
typedef struct gs360_color_plan16 gs360_color_plan16;
int gs360_color_plan16_create(gs360_ctx *ctx, const float *lut, int lut_size, const float *domain_min, const float *domain_max,
                              int n_pieces, const float *piece_start, const int32_t *piece_base, const int32_t *piece_off,
                              const float *thresholds, gs360_color_plan16 **out);
int gs360_color_plan16_destroy(gs360_ctx *ctx, gs360_color_plan16 *plan);
int gs360_color_apply_u16(gs360_ctx *ctx, const gs360_color_plan16 *plan, const void *src, int H, int W, int C,
                          size_t src_stride, int red_index, void *dst, size_t dst_stride, int slot);

/* ---- decoded video frames: Y'CbCr planes -> RGB (VID-COLOR v1) ----------------------------------------------
 * The colour work of gs360_Video2Frames.py's filter `colorspace=iall=bt709:all=smpte170m[:trc=iec61966-2-1]` (V2F:464-466) on
 * device-resident planes: BT.709 Y'CbCr of depth 8 (uint8) or 10 (uint16, value in the low 10 bits, larger samples clamped to 1023),
 * limited or full range -> R'G'B' -> linear light -> SMPTE-C primaries -> sRGB (or, keep_rec709, the Rec.709 curve) -> interleaved
 * RGB, uint8 for depth 8 and uint16 (levels 0..65535) for depth 10.  Chroma is replicated: pixel (x, y) takes the sample
 * (x >> 1, y >> 1) of a 4:2:0 job and (x >> 1, y) of a 4:2:2 job; the chroma planes are ceil(W / 2) wide and, for 4:2:0,
 * ceil(H / 2) high.  Every step is discrete and stated in DESIGN.md 17; tests/vidcolor_np.py restates it and gives the same bytes.
 *   plan   the Y'CbCr -> R'G'B' step is integer arithmetic whose coefficients follow from depth and full_range; the float steps take
 *          three HOST tables that gs360/vidcolor.py builds in float64: primaries = the 3 x 3 matrix (row-major), linear = 16384
 *          floats in [0,1], the Rec.709 linearisation of R'G'B' level i / 16383; encode = 1024 pairs (a, b), the output level at
 *          the lower edge of cell i of sqrt(linear value) * 1024 and its rise over the cell.  keep_rec709 names the curve `encode`
 *          was built for.  A plan serves any number of calls; destroy waits for the device.
 *   jobs   up to GS360_MAX_FRAMES per call; they may differ in size, subsampling and strides (bytes, 0 = tight).  Planes and
 *          destination must not overlap.  Pointers and strides that are all multiples of 4 take the dword path.  Asynchronous on
 *          `slot`.
 *   out    gs360_video_plan_create_out names the destination's depth as well (VID-FEED v1): (depth, out_bits) =
 *          (8, 8) and (10, 16) are what gs360_video_plan_create makes; (10, 8) writes uint8 RGB from 10-bit planes, what the
 *          reference's `format=yuv444p` does inside its filter: the depth-10 integer step and the same `linear` table, an `encode`
 *          table built for levels 0..255.  The destination's row is 3 W samples of out_bits; the encode cells are checked against
 *          the plan's own largest level.
 * Errors, checked for every job before anything is written: GS360_ERR_UNSUPPORTED for a depth other than 8 or 10, for (8, 16) and any
 * out_bits other than 8 or 16, and for another subsampling; GS360_ERR_ARG for NULL pointers, a side outside 1..65535, a stride below
 * its row, an odd address or stride on a side with 16-bit samples (the planes at depth 10, the destination at out_bits 16), more than
 * GS360_MAX_FRAMES jobs, tables with values that are no number or out of range.  Parity with a real ffmpeg's filter is not pinned
 * (no build or test image carries one): the definition is pinned against float64 mathematics (tests/test_vidcolor_cpu.py,
 * tests/test_vidfeed_cpu.py). */
#define GS360_VIDEO_444 0
#define GS360_VIDEO_422 1
#define GS360_VIDEO_420 2
typedef struct gs360_video_job {
    const void *y, *cb, *cr;                    /* H x W, and two chroma planes of the subsampled size */
    size_t y_stride, cb_stride, cr_stride;      /* bytes; 0 = tight */
    int32_t W, H;
    int32_t subsampling;                        /* GS360_VIDEO_4xx */
    int32_t reserved;
    void *dst;                                  /* H x W x 3, uint8 or uint16 */
    size_t dst_stride;                          /* bytes; 0 = tight */
} gs360_video_job;
typedef struct gs360_video_plan gs360_video_plan;
int gs360_video_plan_create(gs360_ctx *ctx, int depth, int full_range, int keep_rec709, const float *primaries,
                            const float *linear, const float *encode, gs360_video_plan **out);
int gs360_video_plan_create_out(gs360_ctx *ctx, int depth, int out_bits, int full_range, int keep_rec709, const float *primaries,
                                const float *linear, const float *encode, gs360_video_plan **out);
int gs360_video_plan_destroy(gs360_ctx *ctx, gs360_video_plan *plan);
int gs360_video_rgb(gs360_ctx *ctx, const gs360_video_plan *plan, const gs360_video_job *jobs, int n_jobs, int slot);

/* ---- decoded fisheye frames: Y'CbCr planes -> a pinhole view in RGB (VID-FISHEYE v1) ------------------------
 * gs360_Video2Frames.py's --fisheye-perspective graph (V2F:467-493), `v360=<fisheye|equisolid>:rectilinear:ih_fov=F:iv_fov=F:
 * h_fov=..:v_fov=..:interp=cubic` followed by the colorspace filter, on device-resident planes in one kernel: every pixel of the
 * S x S view takes its place in the ideal fisheye image (yaw, pitch and roll zero, the lens circle spanning the W x H source), each of
 * the three planes is interpolated there with v360's cubic (4 x 4 taps, 14-bit integer weights, 1/32-px phases, indices clamped to the
 * plane, a subsampled plane at its own coordinate with chroma sample k at luma 2k + 1/2), and the three samples go through
 * gs360_video_rgb's conversion unchanged: interpolate first, convert afterwards, the reference's order.  Pixels whose ray leaves the
 * source are RGB (0, 0, 0).  Every step is discrete and stated in DESIGN.md 18; tests/vidfisheye_np.py restates it and gives the same
 * bytes.  Deviations from the reference's chain: the view is rendered once at S x S in 4:4:4 (the reference renders at v360's default
 * output size with subsampled chroma, then swscale's scale=S:S); 10-bit footage keeps its depth; invisible pixels are black; pixel
 * centres sit at integers (the -1/2 convention of EQ-SPEC).  Parity with a real ffmpeg's v360 is NOT pinned: the definition is pinned
 * against float64 mathematics and hand-derivable answers (tests/test_vidfisheye_cpu.py).
 *   plan   a gs360_video_plan: depth, range, curve and tables as for gs360_video_rgb.
 *   view   the geometry: gs360/vidfisheye.py's view_from_args derives the fields of view as the reference does; the library derives
 *          the kernel's float32 constants from them.
 *   jobs   up to GS360_MAX_FRAMES; every job's W x H is the view's; dst is S x S x 3 (dst_stride 0 = 3 S samples); subsampling and
 *          strides may differ.  Plane pointers and strides that are all multiples of 4 take the dword path.  Asynchronous on `slot`.
 * Errors, checked for the view and every job before anything is written: GS360_ERR_ARG for a NULL view, another projection, S or a
 * source side outside 1..GS360_FISHEYE_MAX_SIDE, input_fov_deg outside [1,360], h_fov_deg or v_fov_deg outside [1,179], a job of
 * another size than the view's, and whatever gs360_video_rgb refuses of a job (with its codes); GS360_ERR_UNSUPPORTED for a plan
 * whose out_bits is not its depth's own (the (10, 8) plans of gs360_video_plan_create_out). */
#define GS360_FISHEYE_EQUIDISTANT 0
#define GS360_FISHEYE_EQUISOLID 1
#define GS360_FISHEYE_MAX_SIDE 16384
typedef struct gs360_video_fisheye_view {
    int32_t projection;                         /* GS360_FISHEYE_EQUIDISTANT | GS360_FISHEYE_EQUISOLID */
    int32_t size;                               /* S: the view is S x S */
    int32_t W, H;                               /* every job's source size */
    double input_fov_deg, h_fov_deg, v_fov_deg; /* the lens circle's field of view; the view's, both axes */
} gs360_video_fisheye_view;
int gs360_video_fisheye_rgb(gs360_ctx *ctx, const gs360_video_plan *plan, const gs360_video_fisheye_view *view,
                            const gs360_video_job *jobs, int n_jobs, int slot);

/* ---- frame sharpness statistics (the FrameSelector's scoring pass) ----------------------------
 * The per-pixel part of score_one_file in cli_tools/gs360_FrameSelector.py (FS:902-1044: gray conversion, fisheye-circle and
 * highlight masks, central crop band) with lapvar32 / tenengrad32 (FS:720-739: cv2.Laplacian ksize 3 + meanStdDev, cv2.Sobel x / y +
 * mean of gx^2 + gy^2) reduced to exact integer sums, and the INTER_AREA downscale fft_energy_fast feeds its FFT (FS:742-786).  The
 * FFT runs on the host or in gs360_frame_fft_energy (below); the masks' branch logic and the final score stay on the host (FS-SPEC
 * v1; gs360/framescore.py).
 *
 * For every frame f < n_frames (H x W x C uint8, C in {1,3,4}, row stride `stride` bytes, 0 = tight; 4-byte aligned base):
 *   gray      C = 1: the sample; else (R*4899 + G*9617 + B*1868 + 8192) >> 14 (cv2 BGR2GRAY on 8U), red at byte red_index (0 or 2)
 *   circle    (2x - (W-1))^2 + (2y - (H-1))^2 <= max(4, min(W,H)^2)     highlight  gray >= 243 (the reference's gray >= 242.25)
 *   band      rows [band_y0, band_y1): the Laplacian [[2,0,2],[0,-8,0],[2,0,2]] and the Sobel pair of the band as an image of its own
 *             (BORDER_REFLECT_101 at its four edges); mag2 = gx^2 + gy^2
 *   valid     (circle, with GS360_FS_CIRCLE) and (not highlight, with GS360_FS_HIGHLIGHTS); all ones without flags
 * stats_dev[f] (device memory) receives the full-frame counts and, over the band, the sums of every band pixel and of its valid
 * pixels.  The call clears the records first.  All sums are integers: the result does not depend on the order of the work.
 * small_dev (NULL = not wanted) holds n_frames device pointers to 2 x small_h x small_w float32 each: plane 0 = the band resized
 * to small_w x small_h with cv2.resize INTER_AREA (OpenCV's per-axis area weights, float32, its operation order), plane 1 = the
 * band's gray at INTER_NEAREST's sample (min(floor(d * s/d_size), s - 1) per axis), from which the host forms the resized mask.
 * small_w <= W and small_h <= band_y1 - band_y0 (equal sizes give the band itself).  n_frames may exceed GS360_MAX_FRAMES (split
 * internally).  H, W <= 65535.  Asynchronous on `slot`. */
#define GS360_FS_CIRCLE 0x1u      /* mask_mode "fisheye_circle" (the pair records, FS:451-455, 693-705) */
#define GS360_FS_HIGHLIGHTS 0x2u  /* ignore_highlights (FS:944-961) */
typedef struct gs360_frame_stats {
    int64_t n_circle, n_highlight, n_highlight_in_circle;      /* whole frame */
    int64_t n, sum_gray, sum_lap, sum_lap2, sum_mag2;          /* every band pixel */
    int64_t n_valid, sum_gray_valid, sum_lap_valid, sum_lap2_valid, sum_mag2_valid;   /* band pixels where `valid` is set */
} gs360_frame_stats;
int gs360_frame_stats_u8(gs360_ctx *ctx, const void *const *frames, int n_frames, int H, int W, int C, size_t stride,
                         int red_index, int band_y0, int band_y1, uint32_t flags, gs360_frame_stats *stats_dev,
                         float *const *small_dev, int small_w, int small_h, int slot);

/* ---- frame edge score (the FrameSelector's default scoring backend) ---------------------------
 * The score of score_one_file_ffmpeg in cli_tools/gs360_FrameSelector.py (FS:789-899: the ffmpeg filter graph format=gray, crop,
 * signalstats, sobel, signalstats, of which the reference reads the two YAVG values), restated as FS-EDGE v1
 * on FS-SPEC's gray.  Frames as gs360_frame_stats_u8 (H x W x C uint8, C in {1,3,4}, `stride` 0 = tight, 4-byte aligned base,
 * red at byte red_index, H, W <= 65535).  For every frame f < n_frames:
 *   band      rows [band_y0, band_y1), full width, an image of its own (the crop filter runs before the edge filter):
 *             n = W * (band_y1 - band_y0), sum_gray = the sum of gray over it
 *   taps      t[row][col], the 3x3 neighbourhood read at mirrored band coordinates m(i, len) = |i| if |i| < len else
 *             2*len - 1 - |i| on both axes (-1 -> 1, len -> len - 1, len = 1 -> 0: not BORDER_REFLECT_101)
 *   edge      ga = -t00 - 2*t01 - t02 + t20 + 2*t21 + t22, gb = -t00 + t02 - 2*t10 + 2*t12 - t20 + t22,
 *             e = min(255, floor(sqrt(ga*ga + gb*gb))) with an exact integer square root; sum_edge = the sum of e over the band
 * out_dev[f] (device memory) receives the three integer sums; the call clears the records first, and the result does not depend
 * on the order of the work.  The host forms the two YAVG values as sum / n (gs360/framescore.py).  n_frames may exceed
 * GS360_MAX_FRAMES (split internally).  Asynchronous on `slot`. */
typedef struct gs360_frame_edge {
    int64_t n, sum_gray, sum_edge;
} gs360_frame_edge;
int gs360_frame_edge_u8(gs360_ctx *ctx, const void *const *frames, int n_frames, int H, int W, int C, size_t stride,
                        int red_index, int band_y0, int band_y1, gs360_frame_edge *out_dev, int slot);

/* ---- frame FFT energy (the fft / hybrid metrics' spectrum term) -------------------------------
 * The FFT of fft_energy_fast in cli_tools/gs360_FrameSelector.py (FS:742-786), on the fft input gs360_frame_stats_u8 writes
 * (FS-FFT v1), so that no plane leaves the device.  For every frame f < n_frames, small_dev[f] is that call's
 * 2 x small_h x small_w float32 output for a frame of H x W with band rows [band_y0, band_y1): plane 0 = g (the INTER_AREA image),
 * plane 1 = the gray at the nearest sample.  With h = small_h, w = small_w, S = fftshift(fft2(g)):
 *   donut   shifted position (i, j) with (i - h/2)^2 + (j - w/2)^2 >= r^2, r = max(1, min(h, w)/8)
 *   valid   at (i, j), the SPATIAL position (the reference multiplies the shifted spectrum by the resized mask): the circle of
 *           gs360_frame_stats_u8 at (xs[j], ys[i]) with GS360_FS_CIRCLE, and plane1[i, j] < 243 with GS360_FS_HIGHLIGHTS;
 *           xs = min(floor(j * W/w), W-1), ys = band_y0 + min(floor(i * bh/h), bh-1) (INTER_NEAREST, bh = band height)
 * out_dev[f] (device memory) receives sum_hf = sum of |S| over the donut, sum_hf_valid = the same over valid positions,
 * n_valid = the count of valid positions (donut or not) and n = h*w.  The host keeps the reference's branches: no mask or
 * n_valid == 0 -> sum_hf / n, else sum_hf_valid / n_valid.  float32 DFT products, double sums, all in a fixed order: the records
 * are bit-identical from call to call, and within 1e-5 relative + 1e-3 absolute of a float64 FFT.  Asynchronous
 * on `slot`, stream-ordered after gs360_frame_stats_u8 on the same slot.  1 <= small_w <= min(W, GS360_FFT_MAX_SIDE),
 * 1 <= small_h <= min(band height, GS360_FFT_MAX_SIDE); n_frames may exceed GS360_MAX_FRAMES (split internally). */
#define GS360_FFT_MAX_SIDE 512
typedef struct gs360_frame_fft {
    double sum_hf, sum_hf_valid;
    int64_t n_valid, n;     /* n = h*w */
} gs360_frame_fft;
int gs360_frame_fft_energy(gs360_ctx *ctx, const float *const *small_dev, int n_frames, int small_w, int small_h, int H, int W,
                           int band_y0, int band_y1, uint32_t flags, gs360_frame_fft *out_dev, int slot);

/* ---- frame optical flow (the FrameSelector's motion pass) -------------------------------------
 * The Lucas-Kanade motion value of _compute_pair_flow_magnitude in cli_tools/gs360_FrameSelector.py (FS:1245-1337, FLOW_METHOD
 * "lucas_kanade"; it replaces _load_flow_gray, cv2.goodFeaturesToTrack and cv2.calcOpticalFlowPyrLK), restated as FS-FLOW v1
 * (DESIGN.md section 10).  frames[f], f < n_frames: H x W x C uint8 (C in {1,3,4}, row stride `stride` bytes, 0 = tight), gray
 * as gs360_frame_stats_u8 (red at byte red_index, 0 or 2).  Each frame that a pair names is, once per call:
 *   cropped   to [crop_x0, crop_x0 + crop_w) x [crop_y0, crop_y0 + crop_h) (the host's copy of FS:1254-1262)
 *   resized   to small_w x small_h <= GS360_FLOW_MAX_SIDE with cv2.resize INTER_AREA on 8U (equal sizes: no resize)
 *   masked    with GS360_FS_CIRCLE: the full-frame circle of gs360_frame_stats_u8 at INTER_NEAREST's sample; used when not empty
 *   cornered  goodFeaturesToTrack(maxCorners 1000, quality 0.01, minDistance 5, blockSize 7, that mask)
 * and pairs[2k], pairs[2k+1] (frame indices, prev then curr) are tracked with calcOpticalFlowPyrLK(winSize 15, maxLevel 2,
 * (EPS|COUNT, 10, 0.03)).  out_dev[k] (device memory) receives the prev frame's corner count, the count of points with status 1
 * and the double sum, in point order, of their float32 |p1 - p0|: the reference's value is sum_mag / n_tracked, None when either
 * count is 0.  points_dev (NULL = not wanted): n_pairs x GS360_FLOW_MAX_CORNERS records, of which the first n_corners of pair k
 * are written.  Every sum runs in a fixed order: records are bit-identical from call to call and do not depend on the other
 * frames or pairs of the call.  n_frames and n_pairs are not limited (frames are computed GS360_MAX_FRAMES per launch and stay
 * resident while later pairs need them).  H, W <= 65535.  Asynchronous on `slot`. */
#define GS360_FLOW_MAX_SIDE 320
#define GS360_FLOW_MAX_CORNERS 1000
typedef struct gs360_frame_flow {
    int64_t n_corners, n_tracked;
    double sum_mag;
} gs360_frame_flow;
typedef struct gs360_flow_point {
    float x0, y0, x1, y1;   /* corner and tracked end point, level-0 pixels */
    int32_t status, pad;
} gs360_flow_point;
int gs360_frame_flow_u8(gs360_ctx *ctx, const void *const *frames, int n_frames, int H, int W, int C, size_t stride,
                        int red_index, int crop_x0, int crop_y0, int crop_w, int crop_h, int small_w, int small_h, uint32_t flags,
                        const int *pairs, int n_pairs, gs360_frame_flow *out_dev, gs360_flow_point *points_dev, int slot);

/* ---- the FrameSelector passes on 16-bit frames (FS-DEPTH16 v1) ----------
 * The three passes above for frames of H x W x C uint16 samples in host byte order (what Video2Frames writes for sources of more
 * than 8 bits per sample): the argument lists of their _u8 twins, `stride` in bytes (0 = tight, W * C * 2; odd strides are taken),
 * base 4-byte aligned for the statistics and the edge pass.
 *   gs360_frame_stats_u16  g16 = the sample (C = 1), else (R*4899 + G*9617 + B*1868 + 8192) >> 14 on the 16-bit samples (cv2
 *       BGR2GRAY on 16U).  Counts, Laplacian, Sobel, band, circle and `valid` as gs360_frame_stats_u8 on the integer g16, with
 *       highlight = g16 >= 62259 (the reference's g16 / 257 >= 242.25).  The sums are exact, in units of 1/257 gray level
 *       (sum_gray, sum_lap) and of 1/257^2 (sum_lap2, sum_mag2); the host divides (gs360/framescore.py, finish(unit=257)).
 *       small_dev: plane 0 = INTER_AREA of the float32 products (float)g16 * (float)(255.0 / 65535.0), in gs360_frame_stats_u8's
 *       order; plane 1 = floor(g16 / 257 + 0.75) = (g16 + 192) / 257 at the nearest sample, the 8-bit level whose `>= 243` is the
 *       highlight test above, so that gs360_frame_fft_energy and the host take the planes as they take the 8-bit ones.
 *       H * W <= GS360_FS16_MAX_PIXELS, else GS360_ERR_UNSUPPORTED before any launch: a pixel adds up to (8 * 65535)^2 to sum_lap2
 *       (columns of 0 and 65535 in turn; sum_mag2's terms stay below 2 * (4 * 65535)^2), and the sums are signed 64-bit.
 *   gs360_frame_edge_u16, gs360_frame_flow_u16  run on the 8-bit view, every sample >> 8, and are FS-EDGE v1 / FS-FLOW v1 from
 *       there: the records (and flow points) are those of the _u8 call on that view. */
#define GS360_FS16_MAX_PIXELS (INT64_MAX / ((int64_t)(8 * 65535) * (8 * 65535)))   /* 33555456: 7680 x 3840 fits */
int gs360_frame_stats_u16(gs360_ctx *ctx, const void *const *frames, int n_frames, int H, int W, int C, size_t stride,
                          int red_index, int band_y0, int band_y1, uint32_t flags, gs360_frame_stats *stats_dev,
                          float *const *small_dev, int small_w, int small_h, int slot);
int gs360_frame_edge_u16(gs360_ctx *ctx, const void *const *frames, int n_frames, int H, int W, int C, size_t stride,
                         int red_index, int band_y0, int band_y1, gs360_frame_edge *out_dev, int slot);
int gs360_frame_flow_u16(gs360_ctx *ctx, const void *const *frames, int n_frames, int H, int W, int C, size_t stride,
                         int red_index, int crop_x0, int crop_y0, int crop_w, int crop_h, int small_w, int small_h, uint32_t flags,
                         const int *pairs, int n_pairs, gs360_frame_flow *out_dev, gs360_flow_point *points_dev, int slot);

/* ---- baseline JPEG scans of device-resident images (JPG-SPEC v1) -------------------------
 * The image writer behind every view of cli_tools/gs360_360PerspCut.py: the `-q:v` / `-huffman optimal` arguments of PC:327-338 and the
 * mjpeg encoder ffmpeg runs for them (the host path hands the same pixels to Pillow, gs360/imageio.py).  For every job an H x W x C
 * uint8 image (C = 1 gray, C = 3 RGB with red at byte 0, written as YCbCr 4:4:4; row stride src_stride bytes, 0 = tight; the buffer
 * rules of the memory section apply) becomes the entropy-coded segment of a baseline sequential JPEG: the Annex K Huffman tables,
 * IJG's scaling of the Annex K quantiser tables for `quality` in 1..100, one block per component in an MCU, restart markers RSTm
 * every restart_interval MCUs (1..65535) and the last interval padded to a byte.  Integer arithmetic throughout: the bytes are a
 * function of the pixels alone.  `out` receives the scan (no header, no EOI: gs360/jpegenc.py builds those), lengths_dev[k] (device
 * memory) its length; a scan longer than out_capacity gets the length UINT64_MAX and none of it is written.  n_jobs may exceed
 * GS360_MAX_VIEWS (split internally); the jobs of a call may differ in size and C.  Asynchronous on `slot`.
 * Errors: GS360_ERR_ARG for sizes outside 1..65535, quality, restart_interval, NULL pointers; GS360_ERR_UNSUPPORTED for other C.
 * gs360_jpeg_scan_bound: *bytes = a capacity no scan of such an image exceeds (416 bytes per block + 3 per restart interval). */
typedef struct gs360_jpeg_job {
    const void *src;       /* H x W x C uint8 */
    int32_t H, W, C;
    size_t src_stride;     /* 0 = tight */
    void *out;             /* the scan */
    size_t out_capacity;
} gs360_jpeg_job;
int gs360_jpeg_scan_u8(gs360_ctx *ctx, const gs360_jpeg_job *jobs, int n_jobs, int quality, int restart_interval,
                       uint64_t *lengths_dev, int slot);
int gs360_jpeg_scan_bound(int H, int W, int C, int restart_interval, size_t *bytes);
/* "JPG-SPEC v1, optimal tables" (DESIGN.md): what `-huffman optimal` asks of the reference's encoder.  gs360_jpeg_scan_opt_u8 is
 * gs360_jpeg_scan_u8 with every image's own Huffman tables: one pass counts the symbols the coder will emit (they depend on
 * restart_interval), one kernel builds the image's four tables by T.81 Annex K.2 as libjpeg implements it (pseudo-symbol 256, ties
 * to the largest index, lengths limited to 16), and the scan is coded with them; nothing leaves the device in between.  tables_dev
 * (device memory) receives n_jobs * 4 * GS360_JPEG_TABLE_BYTES bytes, per image DC0, AC0, DC1, AC1 (the last two all zero for
 * C = 1), each 16 BITS then HUFFVAL, zero padded: the payloads of the file's DHT segments.  An image whose scan exceeds out_capacity
 * still gets its tables.  gs360_jpeg_scan_bound holds (codes stay <= 16 bits).  Errors as gs360_jpeg_scan_u8, and
 * GS360_ERR_UNSUPPORTED for an image of 10^9 or more coefficients (blocks * 64; about 18 000^2 RGB pixels).
 * gs360_jpeg_huff_tables: the table construction alone, hist_dev = n_tables * 256 uint32 symbol counts (each table's sum below 10^9)
 * -> n_tables * GS360_JPEG_TABLE_BYTES bytes; an all-zero histogram gives the all-zero table.  Asynchronous on `slot`. */
#define GS360_JPEG_TABLE_BYTES 272   /* 16 BITS + up to 256 HUFFVAL, zero padded */
int gs360_jpeg_scan_opt_u8(gs360_ctx *ctx, const gs360_jpeg_job *jobs, int n_jobs, int quality, int restart_interval,
                           uint64_t *lengths_dev, uint8_t *tables_dev, int slot);
int gs360_jpeg_huff_tables(gs360_ctx *ctx, const uint32_t *hist_dev, int n_tables, uint8_t *tables_dev, int slot);
/* "JPG-SPEC v1, 4:2:0" (DESIGN.md): the image writer behind the views of cli_tools/gs360_DualFisheyeDistortionCalibration.py,
 * cv2.imwrite(path, image, [IMWRITE_JPEG_QUALITY, q]) at DF:1826-1840, i.e. libjpeg's defaults: 2 x 2 chroma subsampling, the Annex K
 * Huffman tables, any quality 1..100 (the host path gives the same pixels to Pillow's default subsampling).  gs360_jpeg_scan_sub_u8 is
 * the two scan entry points above in one, with a `subsampling` argument: tables_dev == NULL codes with the Annex K tables
 * (gs360_jpeg_scan_u8), tables_dev != NULL with every image's own (gs360_jpeg_scan_opt_u8, 4 * GS360_JPEG_TABLE_BYTES bytes per image;
 * table 0 serves Y, table 1 Cb and Cr); GS360_JPEG_444 gives exactly the bytes of those two.  With GS360_JPEG_420 a C = 3 image's Y, Cb
 * and Cr planes are padded to multiples of 16, Cb and Cr are averaged over 2 x 2 cells as libjpeg's h2v2_downsample does ((a + b + c
 * + d + bias) >> 2, bias 1 at even and 2 at odd output columns), an MCU is 16 x 16 pixels and holds the blocks Y(0,0), Y(0,1), Y(1,0),
 * Y(1,1), Cb, Cr, and restart_interval counts those MCUs; a C = 1 image has no chroma and gets the bytes of GS360_JPEG_444.  The
 * file's SOF0 then gives component 1 the sampling byte 0x22 (gs360/jpegenc.py).  Errors as the two entry points above, and
 * GS360_ERR_ARG for any other `subsampling`.  gs360_jpeg_scan_bound_sub: gs360_jpeg_scan_bound for that mode, 416 bytes per block + 3
 * per restart interval with 6 * ceil(H / 16) * ceil(W / 16) blocks for a C = 3 image under GS360_JPEG_420. */
#define GS360_JPEG_444 0             /* Pillow's numbers for the same modes */
#define GS360_JPEG_420 2
int gs360_jpeg_scan_sub_u8(gs360_ctx *ctx, const gs360_jpeg_job *jobs, int n_jobs, int quality, int restart_interval, int subsampling,
                           uint64_t *lengths_dev, uint8_t *tables_dev, int slot);
int gs360_jpeg_scan_bound_sub(int H, int W, int C, int restart_interval, int subsampling, size_t *bytes);

/* ---- baseline JPEG files decoded on the device (JPD-SPEC v1) -------------------------------------------
 * The inverse of the scans above for the input side: a baseline sequential JPEG (SOF0, 8 bits, one interleaved scan; gray, 4:4:4,
 * 4:2:2, 4:2:0, 4:4:0 or 4:1:1) becomes an H x W x C uint8 image in device memory (C = 3: R, G, B), byte for byte what libjpeg's
 * default decoder returns (islow IDCT, its "fancy" h2v2 / h2v1 / h1v2 upsampling and plain replication for 4:1:1, its fixed-point
 * YCbCr -> RGB tables).  `subsampling` names the luma sampling of a C = 3 file whose chroma components are both sampled 1 x 1:
 * GS360_JPEG_444 1x1, GS360_JPEG_422 2x1 (MCUs of 16 x 8 pixels: Y Y Cb Cr), GS360_JPEG_420 2x2 (16 x 16: Y Y Y Y Cb Cr),
 * GS360_JPEG_440 1x2 (8 x 16: upper Y, lower Y, Cb, Cr) and GS360_JPEG_411 4x1 (32 x 8: Y Y Y Y Cb Cr); a C = 1 job ignores it
 * (its MCU is one block).  restart_interval and the segments' first MCUs count those MCUs.  The encoder entry points above take only
 * GS360_JPEG_444 and GS360_JPEG_420.  The host parses the header (gs360/jpegdec.py) and hands over, all in device memory:
 * `scan`, the entropy-coded segment (everything between the SOS header and EOI, restart markers included); `segments`, per restart interval four uint32: its first byte in `scan`, its length (marker excluded), the number of
 * subsequences of GS360_JPEG_DEC_SUBSEQ_BYTES bytes all earlier intervals take (each ceil(length / that)), and its first MCU (the
 * records are read as 16-byte vectors: `segments` is 16-byte aligned);
 * `tables`, 4 * GS360_JPEG_TABLE_BYTES bytes (DC0, AC0, DC1, AC1: 16 BITS + HUFFVAL, zero padded) followed by four quantiser tables of
 * 64 bytes in file (zig-zag) order; `scratch`, 256-byte aligned, of the size gs360_jpeg_decode_scratch gives for the file (n_subseq:
 * the subsequences of all intervals together).  `out` / out_stride (0 = tight) follow the stride rules of the memory section.
 * status_dev[k] (device memory) is 0 when job k's stream decoded to exactly its blocks and every interval ended at its last byte,
 * 1 when the decoder met an invalid code and 2 when an interval held fewer or more blocks than it should; `out` then holds no image.
 * A truncated or corrupt stream never makes the device read or write outside the job's buffers.  Asynchronous on `slot`.
 * GS360_ERR_UNSUPPORTED: C not 1 or 3, a subsampling that is none of the five GS360_JPEG_4xx values, a table selector above 1 (3 for
 * quantisers); GS360_ERR_ARG: sizes of 2^31 bytes or more, a scratch that is too small or misaligned, misaligned segments. */
#define GS360_JPEG_422 1             /* decoder only (Pillow's number) */
#define GS360_JPEG_440 3             /* decoder only */
#define GS360_JPEG_411 4             /* decoder only */
#define GS360_JPEG_DEC_SUBSEQ_BYTES 128  /* the entropy decoder's unit: one lane decodes one subsequence first */
#define GS360_JPEG_DEC_WG_SUBSEQS 256    /* subsequences one workgroup synchronises among themselves */
typedef struct gs360_jpeg_dec_job {
    const void *scan;
    uint32_t scan_len, n_subseq;                     /* n_subseq: as given to gs360_jpeg_decode_scratch */
    const uint32_t *segments;
    int32_t n_segments;
    const uint8_t *tables;
    int32_t H, W, C, subsampling, restart_interval;  /* restart_interval: MCUs, 0 = none */
    uint8_t comp_tq[4], comp_td[4], comp_ta[4];      /* per component: quantiser, DC and AC table */
    void *scratch;
    size_t scratch_bytes;
    void *out;
    size_t out_stride;
} gs360_jpeg_dec_job;
int gs360_jpeg_decode_u8(gs360_ctx *ctx, const gs360_jpeg_dec_job *jobs, int n_jobs, uint32_t *status_dev, int slot);
int gs360_jpeg_decode_scratch(int H, int W, int C, int subsampling, uint32_t n_subseq, size_t *bytes);
/* The same decode with a gray result, for consumers that never look at colour (the FrameSelector's passes): same jobs, scratch,
 * status codes and argument checks, but `out` is an H x W uint8 plane (out_stride 0 = tight, else at least W).  For a C = 3 job each
 * byte is (4899 R + 9617 G + 1868 B + 8192) >> 14 of the pixel gs360_jpeg_decode_u8 writes for the same file (FS-SPEC's gray, taken
 * after libjpeg's colour conversion and its clamps: not the file's Y plane, which differs from it by rounding); for a C = 1 job it is
 * the Y sample. */
int gs360_jpeg_decode_gray_u8(gs360_ctx *ctx, const gs360_jpeg_dec_job *jobs, int n_jobs, uint32_t *status_dev, int slot);

/* ---- PNG deflate streams of device-resident images (PNG-SPEC v1) ---------------------------------------
 * The PNG writer behind `.png` views and masks (the host path: Pillow at compress_level 3 for 8 bits, gs360/imageio.py's filter-0
 * writer for 16).  For every job an H x W x C image (C = 1, 3 or 4; bytes_per_sample 1 = uint8, 2 = uint16 in host byte order; row
 * stride src_stride bytes, 0 = tight; the buffer rules of the memory section apply) becomes the raw deflate stream of its filtered
 * scanlines: per row the PNG filter with the smallest sum of |residual as int8| (ties to the lower type), 16-bit samples big-endian;
 * the filtered stream in chunks of 65 536 bytes, each one dynamic-Huffman block followed by an empty stored block (so every chunk
 * starts on a byte; the last stored block carries BFINAL); matches only at the distances 1, bpp and 1 + W * bpp, inside segments of
 * 512 bytes, greedy; code lengths limited to 15 bits; a fixed code-length code.  The bytes are a function of the pixels alone
 * (tests/pngenc_np.py restates them).  `out` receives the stream (no zlib header, no Adler-32, no PNG chunks: gs360/pngenc.py builds
 * those), lengths_dev[k] (device memory) its length; a stream longer than out_capacity gets the length UINT64_MAX and none of it is
 * written.  adler_dev (device memory) receives two uint32 per chunk of 65 536 filtered bytes, the jobs' chunks in job order (job k has
 * ceil(H * (1 + W * C * bytes_per_sample) / 65 536)): the sum of the chunk's bytes and the sum of (n - i) * byte i over its n bytes,
 * both mod 65 521, which the host folds into the stream's Adler-32.  n_jobs may exceed GS360_MAX_VIEWS (split internally); the jobs
 * of a call may differ in size, C and depth.  Asynchronous on `slot`.
 * Errors: GS360_ERR_ARG for sides outside 1..65535, NULL pointers, a stride below a row, odd 16-bit addresses or strides;
 * GS360_ERR_UNSUPPORTED for other C or bytes_per_sample.
 * gs360_png_bound (host only): *bytes = a capacity no stream of such an image exceeds (two bytes per filtered byte + 176 per chunk). */
typedef struct gs360_png_job {
    const void *src;       /* H x W x C uint8 or uint16 */
    int32_t H, W, C, bytes_per_sample;
    size_t src_stride;     /* bytes; 0 = tight */
    void *out;             /* the deflate stream */
    size_t out_capacity;
} gs360_png_job;
int gs360_png_deflate(gs360_ctx *ctx, const gs360_png_job *jobs, int n_jobs, uint64_t *lengths_dev, uint32_t *adler_dev, int slot);
int gs360_png_bound(int H, int W, int C, int bytes_per_sample, size_t *bytes);

/* ---- finishing segmentation masks on the device (MSK-SPEC v1) ------------------------------------------
 * What gs360_SegmentationMaskTool.py runs on every image after the network (SEG:680-781), on device-resident data: threshold the raw
 * H x W uint8 mask (`value > thresh`; src NULL = no detection, all clear), close it (dilate, then erode), dilate it, fuse it to the
 * frame edges, OR in the manual add layer (`value > 0`; NULL = none), count the set pixels and write the output.  All steps work on a
 * bit image and are exact; tests/maskfinish_np.py restates them.
 *   elements  given as DATA: `rows` is a HOST array of kh pairs (j1, j2), the half-open span of set columns of element row i, the
 *             anchor is (kw / 2, kh / 2); kh = 0 skips the step.  Dilate ORs, erode ANDs over the offsets (i - kh / 2, j - kw / 2);
 *             pixels outside the image never contribute to a dilate and never restrict an erode.  gs360/maskfinish.py's
 *             structuring_rows builds cv2.getStructuringElement(MORPH_ELLIPSE)'s rows.
 *   fuse      f = fuse (0 skips), s = spread: in every column with a set row among rows [0, f) the rows above the topmost one are
 *             set, likewise below the lowest one of rows [H - f, H); the mask's columns [0, f) and [W - f, W), each spread s rows
 *             up and down, set per row the columns left of the leftmost (right of the rightmost) one.  All four read the mask as it
 *             enters the step.
 *   output    GS360_MASK_OUT_MASK: H x W, `invert ? 0 : 255` where set, else the other; _RGBA: H x W x 4, the image's RGB and that
 *             value as alpha; _KEEP / _REMOVE: H x W x 3, the image where set / not set, zero elsewhere.  A mask without a set pixel
 *             takes the reference's `mask is None` branches: alpha 0 everywhere, the image unchanged.  `image` is H x W x 3 and
 *             needed by all kinds but _MASK.  Strides in bytes, 0 = tight.
 * counts_dev (device memory) receives each job's number of set pixels.  scratch_dev: device memory of at least
 * gs360_mask_finish_scratch's bytes for the same jobs, 256-byte aligned; the call stages the element rows into it and waits for that
 * copy, the kernels are asynchronous on `slot`.  n_jobs may exceed GS360_MAX_VIEWS (split internally); the jobs of a call may differ
 * in everything.
 * Errors: GS360_ERR_UNSUPPORTED for a side above 32768, an element side above 1025, fuse or spread above 1024 (a lane of the side
 * strips reads 2 spread + 1 rows of fuse / 32 dwords); GS360_ERR_ARG for NULL or inconsistent
 * pointers, a stride below a row, a span outside its element, fuse > min(H, W), an unknown kind, a scratch that is too small.
 * Nothing is written then. */
#define GS360_MASK_OUT_MASK 0
#define GS360_MASK_OUT_RGBA 1
#define GS360_MASK_OUT_KEEP 2
#define GS360_MASK_OUT_REMOVE 3
#define GS360_MASK_MAX_SIDE 32768
#define GS360_MASK_MAX_ELEMENT 1025
#define GS360_MASK_MAX_FUSE 1024
typedef struct gs360_mask_job {
    const void *src;            /* H x W uint8 raw mask, or NULL */
    size_t src_stride;
    const void *add;            /* H x W uint8 manual add layer, or NULL */
    size_t add_stride;
    const void *image;          /* H x W x 3 uint8, or NULL for GS360_MASK_OUT_MASK */
    size_t image_stride;
    void *dst;
    size_t dst_stride;
    int32_t H, W, thresh;
    int32_t close_kw, close_kh;
    int32_t expand_kw, expand_kh;
    int32_t fuse, spread;
    int32_t kind, invert;
    int32_t pad;
    const int32_t *close_rows;  /* host memory: close_kh x (j1, j2) */
    const int32_t *expand_rows; /* host memory: expand_kh x (j1, j2) */
} gs360_mask_job;
int gs360_mask_finish_scratch(const gs360_mask_job *jobs, int n_jobs, size_t *bytes);
int gs360_mask_finish_u8(gs360_ctx *ctx, const gs360_mask_job *jobs, int n_jobs, void *scratch_dev, size_t scratch_bytes,
                         uint32_t *counts_dev, int slot);

/* ---- the shadow estimate in front of the finishing chain (MSK-SHADOW v1) -------------------------------
 * estimate_shadow_mask of gs360_SegmentationMaskTool.py (SEG:499-558) between the close and the expansion (SEG:707-724), on
 * device-resident data, in two calls because the element sizes of the second depend on a count the first one leaves:
 *   candidates  P = the raw mask packed at `thresh` and closed (MSK-SPEC steps 0-1); gray (the library's one 8-bit gray), the gray
 *               filtered by the separable symmetric filter `weights` (HOST array of radius + 1 float32, centre outward; border
 *               BORDER_REFLECT_101; row pass then column pass in float32, s = k[0] v(c), s = s + k[i] (v(c - i) + v(c + i)), every
 *               operation rounded on its own) = illum; C0 = gray / (illum + 1e-6f) < t && illum - gray >= delta_min &&
 *               S <= sat_max with cv2's 8-bit RGB2HSV S = (d sdiv[v] + 2048) >> 12 (`sdiv`: HOST array of 256 int32).
 *               counts_dev[k] = count(P).  gs360/maskfinish.py's gaussian_weights and sat_div_table build the two tables.
 *   merge       C1 = C0 & dilate(P, near) & ~P; C2 = open(close(C1, shadow close), open); G = the outermost 8-connected
 *               components of C2 with everything they enclose; clean = the components of G whose doubled area (2 per 2 x 2 cell
 *               of pixel centres with four corners in G, 1 with three) is >= 2 max(1, min_area); M = P | clean goes to dst as
 *               H x W bytes of 0 / 255 and counts_dev[k] = count(M).  The three elements are given as MSK-SPEC's rows (HOST).
 * Both calls take the same jobs (the merge reads H, W, dst, min_area and its elements, the candidates everything else) and the same
 * scratch_dev: device memory of at least gs360_mask_shadow_scratch's bytes, 256-byte aligned, kept between the two calls.  Its
 * layout is fixed so that a test can look at every stage: 256 bytes, then one area per job in job order whose size is what
 * gs360_mask_shadow_scratch gives for that job alone minus 256; an area begins with the bit planes P, C0, C1, C2, clean, each
 * H x ceil(W / 32) dwords rounded up to 256 bytes.  n_jobs may exceed GS360_MAX_VIEWS.  The candidates stage their tables and wait
 * for that copy, the kernels are asynchronous on `slot`; the merge returns when its kernels are done.
 * Errors: GS360_ERR_UNSUPPORTED for a side above 32768, more than 2^30 pixels (labels are 32-bit, areas are doubled), a radius
 * above 255, an element side above 1025; GS360_ERR_ARG as for gs360_mask_finish_u8; GS360_ERR_INTERNAL when a label walk ran past
 * its bound of H W steps (a defect, never data). */
#define GS360_SHADOW_MAX_PIXELS (1 << 30)
#define GS360_SHADOW_MAX_RADIUS 255
typedef struct gs360_shadow_job {
    const void *image;          /* H x W x 3 uint8 RGB */
    size_t image_stride;
    const void *src;            /* H x W uint8 raw mask, or NULL */
    size_t src_stride;
    void *dst;                  /* merge: M, H x W uint8 */
    size_t dst_stride;
    int32_t H, W;
    int32_t thresh;
    int32_t close_kw, close_kh; /* 0 x 0: no close */
    int32_t radius;             /* of the filter: `weights` has radius + 1 entries */
    int32_t sat_max;
    int32_t min_area;           /* merge */
    float t, delta_min;
    int32_t near_kw, near_kh, sclose_kw, sclose_kh, open_kw, open_kh;   /* merge */
    const int32_t *close_rows;  /* host memory: close_kh x (j1, j2) */
    const float *weights;       /* host memory */
    const int32_t *sdiv;        /* host memory */
    const int32_t *near_rows, *sclose_rows, *open_rows;                 /* merge; host memory */
} gs360_shadow_job;
int gs360_mask_shadow_scratch(const gs360_shadow_job *jobs, int n_jobs, size_t *bytes);
int gs360_mask_shadow_candidates_u8(gs360_ctx *ctx, const gs360_shadow_job *jobs, int n_jobs, void *scratch_dev, size_t scratch_bytes,
                                    uint32_t *counts_dev, int slot);
int gs360_mask_shadow_merge_u8(gs360_ctx *ctx, const gs360_shadow_job *jobs, int n_jobs, void *scratch_dev, size_t scratch_bytes,
                               uint32_t *counts_dev, int slot);

/* ---- inpainting the masked region (MSK-INPAINT v1) ------------------------------------------------------
 * apply_mode's `inpaint` of gs360_SegmentationMaskTool.py (SEG:809-815: cv2.inpaint(image, mask, 5, INPAINT_TELEA)) on
 * device-resident data: Telea's weights with a level-ordered march in place of the heap, so that the result depends on no order.
 * `fill` is F, H x W bytes set where > 0 -- what gs360_mask_finish_u8 writes with GS360_MASK_OUT_MASK and invert = 0.  Per pixel of
 * F: d2 = the exact squared distance to the nearest pixel outside F, L = the smallest k with k^2 >= d2, T = sqrtf(d2); the pixels of
 * level k = 1 .. K = max L are computed from the pixels of lower levels within `radius` and written to `image` in place, one launch
 * per level over the batch's list of pixels (DESIGN.md gives the arithmetic op by op; tests/maskinpaint_np.py restates it).  Pixels
 * outside F are never written.  An image whose F is empty or covers it whole is left untouched, with levels_dev[k] = 0.
 * levels_dev (device memory) receives each job's K.  scratch_dev: device memory of at least gs360_mask_inpaint_scratch's bytes for
 * the same jobs, 256-byte aligned.  Per batch of up to GS360_MAX_VIEWS jobs (n_jobs may exceed that) the call reads the batch's
 * level counts back ONCE, with one stream synchronisation, to size the launches of the levels; it reads its error word when the last
 * launch is done and returns then.
 * Errors: GS360_ERR_UNSUPPORTED for a side above 32768, a radius outside 3..8 (below 1 + sqrt 2 a pixel may have no lower level in
 * reach) and for K > 4095 (d2 stays exact in float32, the launches stay bounded; no image is written then); GS360_ERR_ARG for NULL
 * pointers, a stride below a row, a radius below 1, a scratch that is too small; GS360_ERR_INTERNAL when a lane left one of its
 * bounds (a defect, never data). */
#define GS360_INPAINT_MAX_RADIUS 8
#define GS360_INPAINT_MAX_LEVEL 4095
typedef struct gs360_inpaint_job {
    void *image;                /* H x W x 3 uint8 RGB, filled in place */
    size_t image_stride;
    const void *fill;           /* H x W uint8 F */
    size_t fill_stride;
    int32_t H, W;
    int32_t radius;             /* Telea's epsilon: 5 in the reference (SEG:73) */
    int32_t pad;
} gs360_inpaint_job;
int gs360_mask_inpaint_scratch(const gs360_inpaint_job *jobs, int n_jobs, size_t *bytes);
int gs360_mask_inpaint_u8(gs360_ctx *ctx, const gs360_inpaint_job *jobs, int n_jobs, void *scratch_dev, size_t scratch_bytes,
                          uint32_t *levels_dev, int slot);

/* ---- voxel downsampling of a resident point cloud (VOX-SPEC v1) ----------------------------------------
 * gs360_PlyOptimizer.py's compute_point_cloud_stats, _unique_voxel_count and voxel_downsample_by_size (PLY:110-128, 747-862) on a
 * DEVICE array of n x 3 float32 (16-byte aligned) that stays where it is from call to call:
 *   bounds   minmax[0..2] = the per-axis minimum, minmax[3..5] = the maximum (HOST array of six floats).
 *   count    the number of occupied voxels of edge (float) voxel on the grid that starts at minmax[0..2].
 *   pick     *k = that number; pick_dev[0 .. k) = per voxel, in the lexicographic order of the (x, y, z) keys, the original index of
 *            its representative: GS360_VOXEL_FIRST the smallest index, _CENTER / _CENTROID the point nearest the voxel's centre / the
 *            float64 centroid (ties: the smallest index).  order_dev (n) and starts_dev (k of its n entries), when not NULL, receive
 *            the indices in stable key order and where each voxel's segment starts in them; GS360_VOXEL_SEGMENTS writes only these
 *            two (the caller draws its own representative) and takes pick_dev = NULL.  All three are DEVICE arrays of n uint32.
 * minmax is what the bounds call returned for this cloud.  Keys are k_a = floorf((x_a - min_a) / (float) voxel) in float32, as the
 * reference computes them on its float32 arrays.  Count and pick share scratch_dev: device memory of at least gs360_voxel_scratch's
 * bytes, 256-byte aligned.  Every call returns when its result is there.
 * Errors: GS360_ERR_ARG for n < 1, NULL or misaligned pointers, a scratch that is too small, voxel <= 0, a cloud with non-finite
 * coordinates (bounds), a point outside minmax (count, pick); GS360_ERR_UNSUPPORTED for n >= 2^31 and for a voxel so small that the
 * three keys' bit lengths sum to more than 64 or that one key needs more than 63 (the caller counts such a grid on the host);
 * GS360_ERR_INTERNAL when a segment list left its bound (a defect, never data). */
#define GS360_VOXEL_MAX_POINTS 2147483647LL
#define GS360_VOXEL_FIRST 0
#define GS360_VOXEL_CENTER 1
#define GS360_VOXEL_CENTROID 2
#define GS360_VOXEL_SEGMENTS 3
int gs360_voxel_scratch(gs360_ctx *ctx, int64_t n, size_t *bytes);
int gs360_cloud_bounds_f32(gs360_ctx *ctx, const float *xyz_dev, int64_t n, void *scratch_dev, size_t scratch_bytes, float *minmax,
                           int slot);
int gs360_voxel_count_f32(gs360_ctx *ctx, const float *xyz_dev, int64_t n, const float *minmax, double voxel, void *scratch_dev,
                          size_t scratch_bytes, int64_t *count, int slot);
int gs360_voxel_pick_f32(gs360_ctx *ctx, const float *xyz_dev, int64_t n, const float *minmax, double voxel, int strategy,
                         void *scratch_dev, size_t scratch_bytes, uint32_t *pick_dev, uint32_t *order_dev, uint32_t *starts_dev,
                         int64_t *k, int slot);

/* ---- adaptive octree sampling of a resident point cloud (OCT-SPEC v1) ----------------------------------
 * gs360_PlyOptimizer.py's adaptive_voxel_downsample (PLY:1174-1407) on the DEVICE array of n x 3 float32 (16-byte aligned) that the
 * voxel calls take.  The caller computes the cube as the reference does (PLY:1231-1242): cube_size = the largest extent, cube_min
 * (HOST, three floats) = the float32 minimum minus the float32 pad.  A point's path through the octree is a 36-bit code built by
 * the reference's float32 add chain; (code, index) pairs are sorted stably, the split loop runs on the host over counts alone
 * (weights are libm's pow((double) count, weight_power), a negative power counts as 0; min_voxel == 0: none), and the kept leaves
 * are picked on the device over their points in ascending original index.
 *   pick     *k = the number of leaves kept (<= target); pick[0 .. k) (HOST, room for `target`) = per kept leaf, in the reference's
 *            output order (weight, then count, descending; then the smallest index ascending), the original index of its
 *            representative: GS360_VOXEL_FIRST the smallest index, _CENTER / _CENTROID the point nearest the leaf's centre / the
 *            float32 centroid summed in index order (ties: the smallest index).  GS360_VOXEL_SEGMENTS takes pick = NULL and returns
 *            order_dev (DEVICE, n uint32: the indices grouped by leaf, ascending inside a leaf) with starts[0 .. k) and
 *            counts[0 .. k) (HOST, room for `target` each): where each kept leaf lies in order_dev; the caller draws its own
 *            representative.  With another strategy order_dev, starts and counts may be NULL.
 *   stage_ms NULL, or a HOST array of nine doubles that receives the milliseconds of the stages (codes, sort, levels, download,
 *            walk, ordinals, second sort, pick with its download, selection); asking for them drains the stream after every stage.
 * scratch_dev: device memory of at least gs360_octree_scratch's bytes, 256-byte aligned.  The call returns when its result is there.
 * Errors: GS360_ERR_ARG for n < 2, target outside [1, n), NULL or misaligned pointers, a scratch that is too small, a cube that is
 * not finite and positive, a weight power that is not a number; GS360_ERR_UNSUPPORTED for n >= 2^31 and for a weight power at which
 * pow(n, power) is not finite; GS360_ERR_INTERNAL when a leaf list left its bound (a defect, never data). */
int gs360_octree_scratch(gs360_ctx *ctx, int64_t n, size_t *bytes);
int gs360_octree_pick_f32(gs360_ctx *ctx, const float *xyz_dev, int64_t n, const float *cube_min, double cube_size, int64_t target,
                          double weight_power, double min_voxel, int strategy, void *scratch_dev, size_t scratch_bytes,
                          uint32_t *pick, uint32_t *order_dev, uint32_t *starts, uint32_t *counts, int64_t *k, double *stage_ms,
                          int slot);

/* ---- host-buffer conveniences (synchronous: H2D -> kernel -> D2H on `slot`) ----------------- */
int gs360_equirect_views_u8_host(gs360_ctx *ctx, const uint8_t *src, int W, int H, int C, size_t src_stride,
                                 const gs360_view *views, int n_views,
                                 uint8_t *const *dst, size_t dst_stride, int interp, uint32_t flags, int slot);
int gs360_remap_table_u8_host(gs360_ctx *ctx, const uint8_t *src, int H, int W, int C, size_t src_stride,
                              const float *map_x, const float *map_y, const uint8_t *valid, int h, int w,
                              int interp, const double *border_value, int fill_value,
                              uint8_t *dst, size_t dst_stride, int slot);

int gs360_equirect_views_u16_host(gs360_ctx *ctx, const uint16_t *src, int W, int H, int C, size_t src_stride,
                                  const gs360_view *views, int n_views,
                                  uint16_t *const *dst, size_t dst_stride, int interp, uint32_t flags, int slot);
int gs360_remap_table_u16_host(gs360_ctx *ctx, const uint16_t *src, int H, int W, int C, size_t src_stride,
                               const float *map_x, const float *map_y, const uint8_t *valid, int h, int w,
                               int interp, const double *border_value, int fill_value,
                               uint16_t *dst, size_t dst_stride, int slot);

/* ---- self-test ------------------------------------------------------------------------------------------------
 * The kernels evaluate EQ-SPEC / FE-SPEC's divisions and square roots with shorter instruction sequences that are bit-identical
 * to IEEE `/` and sqrt on the specs' operand domains.  This compares both forms on the GPU for n_millions x 10^6 pseudo-random
 * operand sets (and the tiny-operand fallback); *n_mismatch must come back 0. */
int gs360_selftest_arith(gs360_ctx *ctx, uint32_t seed, int n_millions, uint64_t *n_checked, uint64_t *n_mismatch);

/* ---- image-codec helper (host only, no GPU) ------------------------------------------------------
 * In-place PNG scanline reconstruction (filter types 0-4) of h rows of (1 + stride) inflated bytes; bpp = bytes per
 * complete pixel.  Used by the package's own 16-bit PNG reader; image codecs are outside the measured path. */
int gs360_png_unfilter(uint8_t *data, int h, int stride, int bpp);
/* TIFF LZW (compression 5) strip decoder for the package's 16-bit TIFF reader: at most out_cap bytes are produced. */
int gs360_tiff_lzw_decode(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap, size_t *out_len);

#ifdef __cplusplus
}
#endif
#endif /* GS360_H */
