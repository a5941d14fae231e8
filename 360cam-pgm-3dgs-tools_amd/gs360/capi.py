"""ctypes binding of libgs360hip.so (C ABI declared in include/gs360.h).

This is the only door from Python into the engine.  There is NO CPU fallback: if the shared
library or a gfx950 device is missing every call raises Gs360Error.
"""
import ctypes as C
import os
import pathlib
import threading

import numpy as np

PKG_DIR = pathlib.Path(__file__).resolve().parent.parent
LIB_PATH = pathlib.Path(os.environ.get("GS360_LIB", PKG_DIR / "lib" / "libgs360hip.so"))  # override: profiling probes

INTERP_NEAREST = 0  # == cv2.INTER_NEAREST
INTERP_LINEAR = 1   # == cv2.INTER_LINEAR
INTERP_CUBIC = 2    # == cv2.INTER_CUBIC
INTERP_LANCZOS4 = 4  # == cv2.INTER_LANCZOS4 (table remap / fused fisheye only)
EQ_FISHEYE_OUT = 1   # flags: the views are equidistant-fisheye outputs (v360 output=fisheye), see include/gs360.h
MAX_VIEWS = 16
MAX_FRAMES = 16

EXPORTS = (
    "gs360_abi_version", "gs360_device_count", "gs360_last_error", "gs360_ctx_create", "gs360_ctx_destroy",
    "gs360_device_info", "gs360_device_pci_bus_id", "gs360_ctx_set_option", "gs360_ctx_get_option", "gs360_dev_alloc", "gs360_dev_free", "gs360_host_alloc", "gs360_host_free",
    "gs360_upload", "gs360_download", "gs360_dev_memset", "gs360_dev_bswap16", "gs360_sync", "gs360_event_record",
    "gs360_event_elapsed_ms", "gs360_equirect_views_u8", "gs360_equirect_views_masked_u8", "gs360_remap_table_u8",
    "gs360_fisheye_views_u8", "gs360_fisheye_views_border_u8", "gs360_remap_tables_u8", "gs360_map_plan_create", "gs360_map_plan_destroy", "gs360_remap_plans_u8", "gs360_remap_plans_u16",
    "gs360_color_plan_create", "gs360_color_plan_destroy", "gs360_color_apply_u8",
    "gs360_equirect_views_u8_host", "gs360_remap_table_u8_host",
    "gs360_equirect_views_u16", "gs360_remap_table_u16", "gs360_remap_tables_u16", "gs360_equirect_views_u16_host", "gs360_remap_table_u16_host",
    "gs360_png_unfilter", "gs360_event_sync", "gs360_stream_wait_event",
    "gs360_color_plan16_create", "gs360_color_plan16_destroy", "gs360_color_apply_u16", "gs360_tiff_lzw_decode", "gs360_selftest_arith",
    "gs360_frame_stats_u8", "gs360_frame_fft_energy", "gs360_frame_flow_u8", "gs360_frame_edge_u8",
    "gs360_frame_stats_u16", "gs360_frame_edge_u16", "gs360_frame_flow_u16",
    "gs360_jpeg_scan_u8", "gs360_jpeg_scan_bound", "gs360_jpeg_scan_opt_u8", "gs360_jpeg_huff_tables",
    "gs360_jpeg_scan_sub_u8", "gs360_jpeg_scan_bound_sub", "gs360_jpeg_decode_u8", "gs360_jpeg_decode_scratch",
    "gs360_jpeg_decode_gray_u8", "gs360_png_deflate", "gs360_png_bound", "gs360_mask_finish_u8", "gs360_mask_finish_scratch",
    "gs360_mask_shadow_scratch", "gs360_mask_shadow_candidates_u8", "gs360_mask_shadow_merge_u8",
    "gs360_mask_inpaint_scratch", "gs360_mask_inpaint_u8",
    "gs360_voxel_scratch", "gs360_cloud_bounds_f32", "gs360_voxel_count_f32", "gs360_voxel_pick_f32",
    "gs360_octree_scratch", "gs360_octree_pick_f32",
    "gs360_video_plan_create", "gs360_video_plan_destroy", "gs360_video_rgb", "gs360_video_fisheye_rgb",
    "gs360_video_plan_create_out",
)
JPEG_OVERFLOW = 0xFFFFFFFFFFFFFFFF   # a scan length of gs360_jpeg_scan_u8: the scan did not fit its out_capacity
JPEG_TABLE_BYTES = 272               # GS360_JPEG_TABLE_BYTES: one Huffman table of gs360_jpeg_scan_opt_u8 (16 BITS + HUFFVAL, zero padded)
JPEG_444 = 0                         # GS360_JPEG_444 / GS360_JPEG_420: the `subsampling` of gs360_jpeg_scan_sub_u8 (Pillow's numbers)
JPEG_420 = 2
JPEG_422 = 1                         # GS360_JPEG_422 / _440 / _411: further `subsampling` values of gs360_jpeg_decode_u8 (decoder only)
JPEG_440 = 3
JPEG_411 = 4
JPEG_DEC_SUBSEQ_BYTES = 128          # GS360_JPEG_DEC_SUBSEQ_BYTES: bytes of a scan one lane of gs360_jpeg_decode_u8 decodes first
JPEG_DEC_WG_SUBSEQS = 256            # GS360_JPEG_DEC_WG_SUBSEQS: subsequences one workgroup synchronises among themselves
PNG_OVERFLOW = 0xFFFFFFFFFFFFFFFF    # a stream length of gs360_png_deflate: the stream did not fit its out_capacity
PNG_CHUNK = 65536                    # PNG-SPEC v1: filtered bytes per deflate block (and per pair of Adler-32 partial sums)
MASK_OUT_MASK, MASK_OUT_RGBA, MASK_OUT_KEEP, MASK_OUT_REMOVE = 0, 1, 2, 3   # GS360_MASK_OUT_*: the `kind` of gs360_mask_finish_u8
MASK_MAX_SIDE = 32768                # GS360_MASK_MAX_SIDE / GS360_MASK_MAX_ELEMENT: the largest mask side and element side
MASK_MAX_ELEMENT = 1025
MASK_MAX_FUSE = 1024                 # GS360_MASK_MAX_FUSE: the largest edge-fuse strip (and spread)
SHADOW_MAX_PIXELS = 1 << 30          # GS360_SHADOW_MAX_PIXELS / GS360_SHADOW_MAX_RADIUS: the shadow estimate's largest image and filter radius
SHADOW_MAX_RADIUS = 255
INPAINT_MIN_RADIUS, INPAINT_MAX_RADIUS = 3, 8   # gs360_mask_inpaint_u8's radii (GS360_INPAINT_MAX_RADIUS) and its largest K
INPAINT_MAX_LEVEL = 4095             # GS360_INPAINT_MAX_LEVEL
VOXEL_FIRST, VOXEL_CENTER, VOXEL_CENTROID, VOXEL_SEGMENTS = 0, 1, 2, 3   # GS360_VOXEL_*: the `strategy` of gs360_voxel_pick_f32
VOXEL_MAX_POINTS = (1 << 31) - 1     # GS360_VOXEL_MAX_POINTS: indices are 32-bit on the device
VIDEO_444, VIDEO_422, VIDEO_420 = 0, 1, 2   # GS360_VIDEO_*: the `subsampling` of a gs360_video_job
FISHEYE_EQUIDISTANT, FISHEYE_EQUISOLID = 0, 1   # GS360_FISHEYE_*: the `projection` of a gs360_video_fisheye_view
FISHEYE_MAX_SIDE = 16384             # GS360_FISHEYE_MAX_SIDE: the largest source side and view size of gs360_video_fisheye_rgb
ERR_ARG = -1                         # GS360_ERR_ARG / GS360_ERR_UNSUPPORTED
ERR_UNSUPPORTED = -4
ERR_INTERNAL = -6                    # GS360_ERR_INTERNAL: a kernel's own bound was exceeded
FS_CIRCLE = 0x1       # gs360_frame_stats_u8 flags: mask_mode "fisheye_circle"
FS_HIGHLIGHTS = 0x2   # ignore_highlights
FFT_MAX_SIDE = 512    # GS360_FFT_MAX_SIDE: gs360_frame_fft_energy's largest fft input side
FLOW_MAX_SIDE = 320   # GS360_FLOW_MAX_SIDE: gs360_frame_flow_u8's largest small image side (FLOW_DOWNSCALE)
FLOW_MAX_CORNERS = 1000   # GS360_FLOW_MAX_CORNERS: goodFeaturesToTrack's maxCorners
FS16_MAX_PIXELS = (2 ** 63 - 1) // (8 * 65535) ** 2   # GS360_FS16_MAX_PIXELS: gs360_frame_stats_u16's largest H * W (FS-DEPTH16 v1)


class Gs360Error(RuntimeError):
    def __init__(self, code, text):
        super().__init__(f"gs360 error {code}: {text}")
        self.code = code
        self.text = text


class View(C.Structure):
    """Numeric fields of the reference's ViewSpec (gs360_360PerspCut.py:32-45)."""
    _fields_ = [("yaw_deg", C.c_double), ("pitch_deg", C.c_double), ("hfov_deg", C.c_double),
                ("vfov_deg", C.c_double), ("width", C.c_int32), ("height", C.c_int32)]

    @classmethod
    def make(cls, yaw, pitch, hfov, vfov, width, height):
        return cls(float(yaw), float(pitch), float(hfov), float(vfov), int(width), int(height))


class Calib(C.Structure):
    """Numeric fields of the reference's SensorCalibration (gs360_DualFisheyeDistortionCalibration.py:67-85)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32)] + [
        (n, C.c_double) for n in ("f", "cx", "cy", "k1", "k2", "k3", "k4", "p1", "p2", "b1", "b2")]

    @classmethod
    def make(cls, width, height, f, cx=0.0, cy=0.0, k1=0.0, k2=0.0, k3=0.0, k4=0.0, p1=0.0, p2=0.0, b1=0.0, b2=0.0):
        return cls(int(width), int(height), *[float(v) for v in (f, cx, cy, k1, k2, k3, k4, p1, p2, b1, b2)])


class RemapJob(C.Structure):
    """gs360_remap_job: one cv2.remap call of a batched launch (device pointers)."""
    _fields_ = [("src", C.c_void_p), ("H", C.c_int32), ("W", C.c_int32), ("src_stride", C.c_size_t),
                ("map_x", C.c_void_p), ("map_y", C.c_void_p), ("valid", C.c_void_p), ("h", C.c_int32), ("w", C.c_int32),
                ("fill_value", C.c_int32), ("dst", C.c_void_p), ("dst_stride", C.c_size_t)]


class JpegJob(C.Structure):
    """gs360_jpeg_job: one image of a batched JPEG scan call (device pointers)."""
    _fields_ = [("src", C.c_void_p), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("src_stride", C.c_size_t),
                ("out", C.c_void_p), ("out_capacity", C.c_size_t)]


class PngJob(C.Structure):
    """gs360_png_job: one image of a batched PNG deflate call (device pointers)."""
    _fields_ = [("src", C.c_void_p), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("bytes_per_sample", C.c_int32),
                ("src_stride", C.c_size_t), ("out", C.c_void_p), ("out_capacity", C.c_size_t)]


class VideoJob(C.Structure):
    """gs360_video_job: the planes of one decoded frame and its RGB destination (device pointers)."""
    _fields_ = [("y", C.c_void_p), ("cb", C.c_void_p), ("cr", C.c_void_p), ("y_stride", C.c_size_t), ("cb_stride", C.c_size_t),
                ("cr_stride", C.c_size_t), ("W", C.c_int32), ("H", C.c_int32), ("subsampling", C.c_int32), ("reserved", C.c_int32),
                ("dst", C.c_void_p), ("dst_stride", C.c_size_t)]


class VideoFisheyeView(C.Structure):
    """gs360_video_fisheye_view: the geometry of a gs360_video_fisheye_rgb call."""
    _fields_ = [("projection", C.c_int32), ("size", C.c_int32), ("W", C.c_int32), ("H", C.c_int32),
                ("input_fov_deg", C.c_double), ("h_fov_deg", C.c_double), ("v_fov_deg", C.c_double)]


class MaskJob(C.Structure):
    """gs360_mask_job: one mask of a batched finishing call (device pointers; the element rows are host arrays)."""
    _fields_ = [("src", C.c_void_p), ("src_stride", C.c_size_t), ("add", C.c_void_p), ("add_stride", C.c_size_t),
                ("image", C.c_void_p), ("image_stride", C.c_size_t), ("dst", C.c_void_p), ("dst_stride", C.c_size_t),
                ("H", C.c_int32), ("W", C.c_int32), ("thresh", C.c_int32), ("close_kw", C.c_int32), ("close_kh", C.c_int32),
                ("expand_kw", C.c_int32), ("expand_kh", C.c_int32), ("fuse", C.c_int32), ("spread", C.c_int32),
                ("kind", C.c_int32), ("invert", C.c_int32), ("pad", C.c_int32),
                ("close_rows", C.c_void_p), ("expand_rows", C.c_void_p)]


class ShadowJob(C.Structure):
    """gs360_shadow_job: one image of the two shadow-estimate calls (device pointers; the tables and element rows are host arrays)."""
    _fields_ = [("image", C.c_void_p), ("image_stride", C.c_size_t), ("src", C.c_void_p), ("src_stride", C.c_size_t),
                ("dst", C.c_void_p), ("dst_stride", C.c_size_t),
                ("H", C.c_int32), ("W", C.c_int32), ("thresh", C.c_int32), ("close_kw", C.c_int32), ("close_kh", C.c_int32),
                ("radius", C.c_int32), ("sat_max", C.c_int32), ("min_area", C.c_int32), ("t", C.c_float), ("delta_min", C.c_float),
                ("near_kw", C.c_int32), ("near_kh", C.c_int32), ("sclose_kw", C.c_int32), ("sclose_kh", C.c_int32),
                ("open_kw", C.c_int32), ("open_kh", C.c_int32),
                ("close_rows", C.c_void_p), ("weights", C.c_void_p), ("sdiv", C.c_void_p),
                ("near_rows", C.c_void_p), ("sclose_rows", C.c_void_p), ("open_rows", C.c_void_p)]


class InpaintJob(C.Structure):
    """gs360_inpaint_job: one image of a batched inpaint call (device pointers)."""
    _fields_ = [("image", C.c_void_p), ("image_stride", C.c_size_t), ("fill", C.c_void_p), ("fill_stride", C.c_size_t),
                ("H", C.c_int32), ("W", C.c_int32), ("radius", C.c_int32), ("pad", C.c_int32)]


class JpegDecJob(C.Structure):
    """gs360_jpeg_dec_job: one file of a batched JPEG decode call (device pointers)."""
    _fields_ = [("scan", C.c_void_p), ("scan_len", C.c_uint32), ("n_subseq", C.c_uint32), ("segments", C.c_void_p), ("n_segments", C.c_int32),
                ("tables", C.c_void_p), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("subsampling", C.c_int32),
                ("restart_interval", C.c_int32), ("comp_tq", C.c_uint8 * 4), ("comp_td", C.c_uint8 * 4), ("comp_ta", C.c_uint8 * 4),
                ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t), ("out", C.c_void_p), ("out_stride", C.c_size_t)]


class FrameStats(C.Structure):
    """gs360_frame_stats: full-frame mask counts and the band's exact sums (all band pixels, then the valid ones)."""
    _fields_ = [(n, C.c_int64) for n in (
        "n_circle", "n_highlight", "n_highlight_in_circle", "n", "sum_gray", "sum_lap", "sum_lap2", "sum_mag2",
        "n_valid", "sum_gray_valid", "sum_lap_valid", "sum_lap2_valid", "sum_mag2_valid")]


class FrameEdge(C.Structure):
    """gs360_frame_edge: the band's pixel count and its exact sums of gray and of the clipped Sobel magnitude (FS-EDGE v1)."""
    _fields_ = [("n", C.c_int64), ("sum_gray", C.c_int64), ("sum_edge", C.c_int64)]


class FrameFft(C.Structure):
    """gs360_frame_fft: sum of |fftshift(fft2(g))| over the donut, over the donut's valid positions, the valid count and h*w."""
    _fields_ = [("sum_hf", C.c_double), ("sum_hf_valid", C.c_double), ("n_valid", C.c_int64), ("n", C.c_int64)]


class FrameFlow(C.Structure):
    """gs360_frame_flow: the prev frame's corner count, the tracked (status 1) count and the double sum of their |p1 - p0|."""
    _fields_ = [("n_corners", C.c_int64), ("n_tracked", C.c_int64), ("sum_mag", C.c_double)]


class FlowPoint(C.Structure):
    """gs360_flow_point: one corner, its tracked end point (level-0 pixels) and its status."""
    _fields_ = [("x0", C.c_float), ("y0", C.c_float), ("x1", C.c_float), ("y1", C.c_float), ("status", C.c_int32), ("pad", C.c_int32)]


_NP_OF_C = {C.c_double: np.float64, C.c_int64: np.int64, C.c_int32: np.int32, C.c_float: np.float32}


def record_dtype(struct):
    """The NumPy dtype of a ctypes record of c_double / c_int64 / c_int32 / c_float fields, with the same field names and bytes."""
    dt = np.dtype([(n, _NP_OF_C[t]) for n, t in struct._fields_])
    assert dt.itemsize == C.sizeof(struct), struct.__name__
    return dt


ABI_VERSION = 2          # GS360_ABI_VERSION of include/gs360.h this binding was written against
_lib = None
_lib_lock = threading.Lock()


def load_library(path=None):
    """Load libgs360hip.so and declare prototypes.  Raises Gs360Error if it is not built."""
    global _lib
    with _lib_lock:
        if _lib is not None and path is None:
            return _lib
        p = pathlib.Path(path) if path else LIB_PATH
        if not p.exists():
            raise Gs360Error(-3, f"{p} is missing -- build it with `python __graft_entry__.py` "
                                 "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        L = C.CDLL(str(p))
        # the version first: a stale library should say so, not fail on a symbol it does not have yet
        try:
            L.gs360_abi_version.argtypes = []
            have = int(L.gs360_abi_version())
        except AttributeError:
            have = -1
        if have != ABI_VERSION:
            raise Gs360Error(-4, f"{p} has C-ABI version {have}, this binding needs {ABI_VERSION} (include/gs360.h): rebuild it with "
                                 "`python __graft_entry__.py`")
        vp, i, sz, u32 = C.c_void_p, C.c_int, C.c_size_t, C.c_uint32
        pvp = C.POINTER(C.c_void_p)
        L.gs360_abi_version.argtypes = []
        L.gs360_device_count.argtypes = []
        L.gs360_last_error.argtypes = [C.c_char_p, sz]
        L.gs360_ctx_create.argtypes = [i, i, pvp]
        L.gs360_ctx_destroy.argtypes = [vp]
        L.gs360_device_info.argtypes = [vp, C.c_char_p, sz, C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]
        L.gs360_device_pci_bus_id.argtypes = [vp, C.c_char_p, sz]
        L.gs360_ctx_set_option.argtypes = [vp, C.c_char_p, i]
        L.gs360_ctx_get_option.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int)]
        L.gs360_dev_alloc.argtypes = [vp, sz, pvp]
        L.gs360_dev_free.argtypes = [vp, vp]
        L.gs360_host_alloc.argtypes = [vp, sz, pvp]
        L.gs360_host_free.argtypes = [vp, vp]
        L.gs360_upload.argtypes = [vp, vp, vp, sz, i]
        L.gs360_download.argtypes = [vp, vp, vp, sz, i]
        L.gs360_dev_memset.argtypes = [vp, vp, i, sz, i]
        L.gs360_dev_bswap16.argtypes = [vp, vp, sz, i]
        L.gs360_sync.argtypes = [vp, i]
        L.gs360_event_record.argtypes = [vp, i, i]
        L.gs360_event_elapsed_ms.argtypes = [vp, i, i, i, C.POINTER(C.c_float)]
        L.gs360_equirect_views_u8.argtypes = [vp, pvp, i, i, i, i, sz, C.POINTER(View), i, pvp, sz, i, u32, i]
        L.gs360_equirect_views_masked_u8.argtypes = [vp, pvp, pvp, i, i, i, i, sz, sz, C.POINTER(View), i, pvp, sz, i, u32, i]
        L.gs360_remap_table_u8.argtypes = [vp, vp, i, i, i, sz, vp, vp, vp, i, i, i, C.POINTER(C.c_double), i, vp, sz, i]
        L.gs360_fisheye_views_u8.argtypes = [vp, pvp, C.POINTER(Calib), i, sz, C.POINTER(View), i, C.c_double, i, i, i,
                                             pvp, sz, pvp, i]
        L.gs360_fisheye_views_border_u8.argtypes = [vp, pvp, C.POINTER(Calib), i, sz, C.POINTER(View), i, C.c_double, i, i, i,
                                                    C.POINTER(C.c_double), pvp, sz, pvp, i]
        L.gs360_remap_tables_u8.argtypes = [vp, C.POINTER(RemapJob), i, i, i, C.POINTER(C.c_double), i]
        L.gs360_map_plan_create.argtypes = [vp, vp, vp, vp, i, i, i, i, pvp]
        L.gs360_map_plan_destroy.argtypes = [vp, vp]
        L.gs360_remap_plans_u8.argtypes = [vp, C.POINTER(RemapJob), pvp, i, i, i, C.POINTER(C.c_double), i]
        L.gs360_remap_plans_u16.argtypes = L.gs360_remap_plans_u8.argtypes
        L.gs360_color_plan_create.argtypes = [vp, vp, i, vp, vp, pvp]
        L.gs360_color_plan_destroy.argtypes = [vp, vp]
        L.gs360_color_apply_u8.argtypes = [vp, vp, vp, i, i, i, sz, i, vp, sz, i]
        L.gs360_equirect_views_u8_host.argtypes = [vp, vp, i, i, i, sz, C.POINTER(View), i, pvp, sz, i, u32, i]
        L.gs360_remap_table_u8_host.argtypes = [vp, vp, i, i, i, sz, vp, vp, vp, i, i, i, C.POINTER(C.c_double), i, vp,
                                                sz, i]
        L.gs360_equirect_views_u16.argtypes = L.gs360_equirect_views_u8.argtypes
        L.gs360_remap_table_u16.argtypes = L.gs360_remap_table_u8.argtypes
        L.gs360_remap_tables_u16.argtypes = L.gs360_remap_tables_u8.argtypes
        L.gs360_equirect_views_u16_host.argtypes = L.gs360_equirect_views_u8_host.argtypes
        L.gs360_remap_table_u16_host.argtypes = L.gs360_remap_table_u8_host.argtypes
        L.gs360_png_unfilter.argtypes = [vp, i, i, i]
        L.gs360_selftest_arith.argtypes = [vp, u32, i, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.gs360_tiff_lzw_decode.argtypes = [vp, sz, vp, sz, C.POINTER(C.c_size_t)]
        L.gs360_color_plan16_create.argtypes = [vp, vp, i, vp, vp, i, vp, vp, vp, vp, pvp]
        L.gs360_color_plan16_destroy.argtypes = [vp, vp]
        L.gs360_color_apply_u16.argtypes = [vp, vp, vp, i, i, i, sz, i, vp, sz, i]
        L.gs360_event_sync.argtypes = [vp, i, i]
        L.gs360_stream_wait_event.argtypes = [vp, i, i, i]
        L.gs360_frame_stats_u8.argtypes = [vp, pvp, i, i, i, i, sz, i, i, i, u32, vp, pvp, i, i, i]
        L.gs360_frame_edge_u8.argtypes = [vp, pvp, i, i, i, i, sz, i, i, i, vp, i]
        L.gs360_frame_stats_u16.argtypes = L.gs360_frame_stats_u8.argtypes
        L.gs360_frame_edge_u16.argtypes = L.gs360_frame_edge_u8.argtypes
        L.gs360_frame_fft_energy.argtypes = [vp, pvp, i, i, i, i, i, i, i, u32, vp, i]
        L.gs360_frame_flow_u8.argtypes = [vp, pvp, i, i, i, i, sz, i, i, i, i, i, i, i, u32, C.POINTER(C.c_int), i, vp, vp, i]
        L.gs360_frame_flow_u16.argtypes = L.gs360_frame_flow_u8.argtypes
        L.gs360_jpeg_scan_u8.argtypes = [vp, C.POINTER(JpegJob), i, i, i, vp, i]
        L.gs360_jpeg_scan_bound.argtypes = [i, i, i, i, C.POINTER(C.c_size_t)]
        L.gs360_jpeg_scan_opt_u8.argtypes = [vp, C.POINTER(JpegJob), i, i, i, vp, vp, i]
        L.gs360_jpeg_huff_tables.argtypes = [vp, vp, i, vp, i]
        L.gs360_jpeg_scan_sub_u8.argtypes = [vp, C.POINTER(JpegJob), i, i, i, i, vp, vp, i]
        L.gs360_jpeg_scan_bound_sub.argtypes = [i, i, i, i, i, C.POINTER(C.c_size_t)]
        L.gs360_jpeg_decode_u8.argtypes = [vp, C.POINTER(JpegDecJob), i, vp, i]
        L.gs360_jpeg_decode_gray_u8.argtypes = [vp, C.POINTER(JpegDecJob), i, vp, i]
        L.gs360_jpeg_decode_scratch.argtypes = [i, i, i, i, u32, C.POINTER(C.c_size_t)]
        L.gs360_png_deflate.argtypes = [vp, C.POINTER(PngJob), i, vp, vp, i]
        L.gs360_png_bound.argtypes = [i, i, i, i, C.POINTER(C.c_size_t)]
        L.gs360_mask_finish_scratch.argtypes = [C.POINTER(MaskJob), i, C.POINTER(C.c_size_t)]
        L.gs360_mask_finish_u8.argtypes = [vp, C.POINTER(MaskJob), i, vp, sz, vp, i]
        L.gs360_mask_shadow_scratch.argtypes = [C.POINTER(ShadowJob), i, C.POINTER(C.c_size_t)]
        L.gs360_mask_shadow_candidates_u8.argtypes = [vp, C.POINTER(ShadowJob), i, vp, sz, vp, i]
        L.gs360_mask_shadow_merge_u8.argtypes = [vp, C.POINTER(ShadowJob), i, vp, sz, vp, i]
        L.gs360_mask_inpaint_scratch.argtypes = [C.POINTER(InpaintJob), i, C.POINTER(C.c_size_t)]
        L.gs360_mask_inpaint_u8.argtypes = [vp, C.POINTER(InpaintJob), i, vp, sz, vp, i]
        i64 = C.c_int64
        L.gs360_voxel_scratch.argtypes = [vp, i64, C.POINTER(C.c_size_t)]
        L.gs360_cloud_bounds_f32.argtypes = [vp, vp, i64, vp, sz, C.POINTER(C.c_float), i]
        L.gs360_voxel_count_f32.argtypes = [vp, vp, i64, C.POINTER(C.c_float), C.c_double, vp, sz, C.POINTER(i64), i]
        L.gs360_voxel_pick_f32.argtypes = [vp, vp, i64, C.POINTER(C.c_float), C.c_double, i, vp, sz, vp, vp, vp, C.POINTER(i64), i]
        L.gs360_octree_scratch.argtypes = [vp, i64, C.POINTER(C.c_size_t)]
        L.gs360_octree_pick_f32.argtypes = [vp, vp, i64, C.POINTER(C.c_float), C.c_double, i64, C.c_double, C.c_double, i, vp, sz, vp, vp, vp, vp,
                                            C.POINTER(i64), C.POINTER(C.c_double), i]
        L.gs360_video_plan_create.argtypes = [vp, i, i, i, vp, vp, vp, pvp]
        L.gs360_video_plan_create_out.argtypes = [vp, i, i, i, i, vp, vp, vp, pvp]
        L.gs360_video_plan_destroy.argtypes = [vp, vp]
        L.gs360_video_rgb.argtypes = [vp, vp, C.POINTER(VideoJob), i, i]
        L.gs360_video_fisheye_rgb.argtypes = [vp, vp, C.POINTER(VideoFisheyeView), C.POINTER(VideoJob), i, i]
        for name in EXPORTS:
            getattr(L, name).restype = C.c_int
        if path is None:
            _lib = L
        return L


def last_error(L=None):
    L = L or load_library()
    buf = C.create_string_buffer(512)
    L.gs360_last_error(buf, 512)
    return buf.value.decode(errors="replace")


def _check(rc, L):
    if rc != 0:
        raise Gs360Error(rc, last_error(L))


def device_count():
    return load_library().gs360_device_count()


class DeviceBuffer:
    """A device allocation owned by a Context (freed with the context or explicitly)."""

    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        _check(ctx.L.gs360_dev_alloc(ctx.handle, self.nbytes, C.byref(p)), ctx.L)
        self.ptr = p.value

    def free(self):
        if self.ptr:
            self.ctx.L.gs360_dev_free(self.ctx.handle, self.ptr)
            self.ptr = None


class PinnedBuffer:
    """Page-locked host memory (gs360_host_alloc): async copies to/from it overlap with kernels."""

    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        _check(ctx.L.gs360_host_alloc(ctx.handle, self.nbytes, C.byref(p)), ctx.L)
        self.ptr = p.value
        self.view = (C.c_uint8 * self.nbytes).from_address(self.ptr)   # writable buffer for numpy.frombuffer

    def free(self):
        if self.ptr:
            self.view = None
            self.ctx.L.gs360_host_free(self.ctx.handle, self.ptr)
            self.ptr = None


class Context:
    """One engine context = one GPU + n_slots HIP streams.  Thread-safe per slot (a lock per slot)."""

    def __init__(self, device=0, n_slots=2):
        self.L = load_library()
        h = C.c_void_p()
        _check(self.L.gs360_ctx_create(int(device), int(n_slots), C.byref(h)), self.L)
        self.handle = h
        self.device = int(device)
        self.n_slots = int(n_slots)
        self.slot_locks = [threading.Lock() for _ in range(n_slots)]
        self._buffers = set()                 # live DeviceBuffers; touched by reader and render threads alike
        self._buffers_lock = threading.Lock()

    # -- lifetime ---------------------------------------------------------------------------
    def close(self):
        if self.handle:
            with self._buffers_lock:
                live, self._buffers = self._buffers, set()
            for b in live:
                b.free()
            self.L.gs360_ctx_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def info(self):
        name = C.create_string_buffer(256)
        cu = C.c_int32()
        mem = C.c_uint64()
        _check(self.L.gs360_device_info(self.handle, name, 256, C.byref(cu), C.byref(mem)), self.L)
        return {"name": name.value.decode(), "cu_count": cu.value, "hbm_bytes": mem.value}

    # -- memory -----------------------------------------------------------------------------
    def alloc(self, nbytes):
        b = DeviceBuffer(self, nbytes)
        with self._buffers_lock:
            self._buffers.add(b)
        return b

    def free(self, buf):
        buf.free()
        with self._buffers_lock:
            self._buffers.discard(buf)

    def pinned(self, nbytes):
        return PinnedBuffer(self, nbytes)

    def unpin(self, hbuf):
        hbuf.free()

    def upload(self, buf, array, slot=0, sync=True):
        a = np.ascontiguousarray(array)
        if a.nbytes > buf.nbytes:
            raise ValueError("upload larger than buffer")
        _check(self.L.gs360_upload(self.handle, buf.ptr, a.ctypes.data, a.nbytes, slot), self.L)
        if sync:
            self.sync(slot)
        return buf

    def to_device(self, array, slot=0):
        a = np.ascontiguousarray(array)
        return self.upload(self.alloc(a.nbytes), a, slot)

    def download(self, buf, shape, dtype=np.uint8, slot=0):
        out = np.empty(shape, dtype=dtype)
        if out.nbytes > buf.nbytes:
            raise ValueError("download larger than buffer")
        _check(self.L.gs360_download(self.handle, out.ctypes.data, buf.ptr, out.nbytes, slot), self.L)
        self.sync(slot)
        return out

    def memset(self, buf, value, slot=0):
        _check(self.L.gs360_dev_memset(self.handle, buf.ptr, int(value), buf.nbytes, slot), self.L)

    def bswap16(self, buf, n_samples, slot=0):
        """in-place byte swap of 16-bit samples on the device (asynchronous on `slot`)"""
        _check(self.L.gs360_dev_bswap16(self.handle, buf.ptr, int(n_samples), slot), self.L)

    def sync(self, slot=-1):
        _check(self.L.gs360_sync(self.handle, slot), self.L)

    def pci_bus_id(self):
        """'domain:bus:device.function' of this context's GPU"""
        buf = C.create_string_buffer(64)
        _check(self.L.gs360_device_pci_bus_id(self.handle, buf, 64), self.L)
        return buf.value.decode()

    def set_option(self, key, value):
        """kernel-selection switch of this context (include/gs360.h: gs360_ctx_set_option); results never depend on it"""
        _check(self.L.gs360_ctx_set_option(self.handle, key.encode(), int(value)), self.L)

    def get_option(self, key):
        v = C.c_int(0)
        _check(self.L.gs360_ctx_get_option(self.handle, key.encode(), C.byref(v)), self.L)
        return int(v.value)

    def options(self, **kw):
        """context manager: set options, restore the previous values on exit (tests)"""
        ctx = self

        class _Scope:
            def __enter__(self_inner):
                self_inner.old = {k: ctx.get_option(k) for k in kw}
                for k, v in kw.items():
                    ctx.set_option(k, v)
                return ctx

            def __exit__(self_inner, *exc):
                for k, v in self_inner.old.items():
                    ctx.set_option(k, v)
                return False
        return _Scope()

    def event_record(self, slot, idx):
        _check(self.L.gs360_event_record(self.handle, slot, idx), self.L)

    def selftest_arith(self, seed=1, n_millions=256):
        """-> (operand sets checked, mismatches) of the reduced division / square-root sequences against IEEE `/`, sqrt"""
        n, bad = C.c_uint64(0), C.c_uint64(0)
        _check(self.L.gs360_selftest_arith(self.handle, int(seed) & 0xFFFFFFFF, int(n_millions), C.byref(n), C.byref(bad)), self.L)
        return int(n.value), int(bad.value)

    def event_sync(self, slot, idx):
        _check(self.L.gs360_event_sync(self.handle, slot, idx), self.L)

    def stream_wait_event(self, waiting_slot, event_slot, idx):
        _check(self.L.gs360_stream_wait_event(self.handle, waiting_slot, event_slot, idx), self.L)

    def event_elapsed_ms(self, slot, i_from, i_to):
        ms = C.c_float()
        _check(self.L.gs360_event_elapsed_ms(self.handle, slot, i_from, i_to, C.byref(ms)), self.L)
        return float(ms.value)

    # -- hot path, device-resident ----------------------------------------------------------
    def equirect_views_dev(self, frames, W, H, Cn, views, dsts, slot=0, src_stride=0, dst_stride=0,
                           interp=INTERP_LINEAR, masks=None, flags=0, dtype=np.uint8):
        """frames: list of DeviceBuffer (H x W x C); dsts: list (len frames*views) of DeviceBuffer;
        masks: optional list of DeviceBuffer (H x W u8 keep-masks, one per frame) fused into the output.
        dtype: np.uint8 or np.uint16 samples (strides in bytes)."""
        nf, nv = len(frames), len(views)
        fp = (C.c_void_p * max(nf, 1))(*[b.ptr for b in frames])
        dp = (C.c_void_p * max(nf * nv, 1))(*[b.ptr for b in dsts])
        va = (View * max(nv, 1))(*views)
        if masks is not None:
            if len(masks) != nf:
                raise ValueError("one mask per frame")
            if np.dtype(dtype) != np.uint8:
                raise Gs360Error(-4, "the fused keep-mask exists for 8-bit images only")
            mp = (C.c_void_p * max(nf, 1))(*[b.ptr for b in masks])
            _check(self.L.gs360_equirect_views_masked_u8(self.handle, fp, mp, nf, W, H, Cn, src_stride, 0, va, nv, dp,
                                                         dst_stride, interp, int(flags), slot), self.L)
            return
        fn = self.L.gs360_equirect_views_u16 if np.dtype(dtype) == np.uint16 else self.L.gs360_equirect_views_u8
        _check(fn(self.handle, fp, nf, W, H, Cn, src_stride, va, nv, dp, dst_stride, interp, int(flags), slot), self.L)

    def make_equirect_call(self, frames, W, H, Cn, views, dsts, slot=0, interp=INTERP_LINEAR, src_stride=0):
        """Pre-marshal one batched launch; returns a zero-argument callable (used by bench loops)."""
        nf, nv = len(frames), len(views)
        fp = (C.c_void_p * nf)(*[b.ptr for b in frames])
        dp = (C.c_void_p * (nf * nv))(*[b.ptr for b in dsts])
        va = (View * nv)(*views)
        fn, h, L = self.L.gs360_equirect_views_u8, self.handle, self.L

        def call():
            rc = fn(h, fp, nf, W, H, Cn, int(src_stride), va, nv, dp, 0, int(interp), 0, slot)
            if rc:
                _check(rc, L)
        call.keepalive = (fp, dp, va)
        return call

    def remap_table_dev(self, src, H, W, Cn, map_x, map_y, valid, h, w, dst, interp=INTERP_LINEAR,
                        border_value=(0, 0, 0, 0), fill_value=0, slot=0, dtype=np.uint8):
        bv = (C.c_double * 4)(*[float(x) for x in border_value])
        fn = self.L.gs360_remap_table_u16 if np.dtype(dtype) == np.uint16 else self.L.gs360_remap_table_u8
        _check(fn(self.handle, src.ptr, H, W, Cn, 0, map_x.ptr, map_y.ptr, valid.ptr if valid is not None else None, h, w, interp, bv,
                  int(fill_value), dst.ptr, 0, slot), self.L)

    def remap_tables_dev(self, jobs, Cn, interp=INTERP_LINEAR, border_value=(0, 0, 0, 0), slot=0, dtype=np.uint8):
        """Several remaps in one launch.  jobs: iterable of (src, H, W, map_x, map_y, valid_or_None, h, w, fill_value, dst)
        with DeviceBuffer objects for src / maps / valid / dst."""
        arr = (RemapJob * len(jobs))()
        for k, (src, H, W, mx, my, valid, h, w, fill, dst) in enumerate(jobs):
            arr[k] = RemapJob(src.ptr, H, W, 0, mx.ptr, my.ptr, valid.ptr if valid is not None else None, h, w, int(fill), dst.ptr, 0)
        bv = (C.c_double * 4)(*[float(x) for x in border_value])
        fn = self.L.gs360_remap_tables_u16 if np.dtype(dtype) == np.uint16 else self.L.gs360_remap_tables_u8
        _check(fn(self.handle, arr, len(jobs), Cn, interp, bv, slot), self.L)

    # -- map plans: the float maps of a run packed once (include/gs360.h) -------------------------
    MAP_PLAN_MAX_DIM = 4079

    def map_plan(self, map_x, map_y, valid, h, w, nearest=False, slot=0):
        """DeviceBuffers holding h x w float32 maps (+ uint8 valid or None) -> plan handle; the buffers may be freed afterwards."""
        hnd = C.c_void_p()
        _check(self.L.gs360_map_plan_create(self.handle, map_x.ptr, map_y.ptr, valid.ptr if valid is not None else None, int(h), int(w),
                                            1 if nearest else 0, slot, C.byref(hnd)), self.L)
        return hnd

    def map_plan_free(self, plan):
        if plan:
            _check(self.L.gs360_map_plan_destroy(self.handle, plan), self.L)

    def remap_plans_dev(self, jobs, Cn, interp=INTERP_LINEAR, border_value=(0, 0, 0, 0), slot=0, dtype=np.uint8):
        """remap_tables_dev with plans: jobs = iterable of (src, H, W, plan, use_valid, h, w, fill_value, dst)."""
        n = len(jobs)
        arr = (RemapJob * n)()
        pl = (C.c_void_p * n)()
        for k, (src, H, W, plan, use_valid, h, w, fill, dst) in enumerate(jobs):
            # valid: any non-NULL value asks for the plan's valid bit; the pointer is not read
            arr[k] = RemapJob(src.ptr, H, W, 0, None, None, dst.ptr if use_valid else None, h, w, int(fill), dst.ptr, 0)
            pl[k] = plan
        bv = (C.c_double * 4)(*[float(x) for x in border_value])
        fn = self.L.gs360_remap_plans_u16 if np.dtype(dtype) == np.uint16 else self.L.gs360_remap_plans_u8
        _check(fn(self.handle, arr, pl, n, Cn, interp, bv, slot), self.L)

    def fisheye_views_dev(self, lens_bufs, calibs, Cn, views, lens_fov_deg, dsts, valid_outs=None,
                          interp=INTERP_LINEAR, mask_outside=True, mask_value=0, slot=0, src_stride=0, dst_stride=0, border_value=None):
        """lens_bufs / dsts / valid_outs: DeviceBuffer objects or raw device addresses (buf.ptr + offset), None = NULL; strides in
        bytes, 0 = tight.  border_value: the border taps' colour per channel in memory order (gs360_fisheye_views_border_u8), None =
        (mask_value, 0, 0, 0)."""
        def addr(b):
            return b if b is None or isinstance(b, int) else b.ptr
        nv = len(views)
        sp = (C.c_void_p * nv)(*[addr(b) for b in lens_bufs])
        dp = (C.c_void_p * nv)(*[addr(b) for b in dsts])
        vo = (C.c_void_p * nv)(*[addr(b) for b in valid_outs]) if valid_outs else None
        ca = (Calib * nv)(*calibs)
        va = (View * nv)(*views)
        head = (self.handle, sp, ca, Cn, int(src_stride), va, nv, float(lens_fov_deg), interp, 1 if mask_outside else 0, int(mask_value))
        tail = (dp, int(dst_stride), vo, slot)
        if border_value is None:
            _check(self.L.gs360_fisheye_views_u8(*head, *tail), self.L)
        else:
            bv = (C.c_double * 4)(*[float(x) for x in border_value])
            _check(self.L.gs360_fisheye_views_border_u8(*head, bv, *tail), self.L)

    # -- input colour stage ------------------------------------------------------------------
    @staticmethod
    def _color_lut(lut_table):
        lut = np.ascontiguousarray(lut_table, dtype=np.float32)
        if lut.ndim != 4 or lut.shape[3] != 3 or not (lut.shape[0] == lut.shape[1] == lut.shape[2]):
            raise ValueError("lut_table must be [n][n][n][3]")
        return lut

    def color_plan(self, lut_table, level_pos, out_thresholds):
        """lut_table: float32 [n][n][n][3] ([b][g][r], .cube order); level_pos: float32 [3][256]; out_thresholds:
        float32 [256] (entry 0 unused).  Returns an opaque plan handle (free with color_plan_free)."""
        lut = self._color_lut(lut_table)
        pos = np.ascontiguousarray(level_pos, dtype=np.float32)
        thr = np.ascontiguousarray(out_thresholds, dtype=np.float32)
        if pos.shape != (3, 256) or thr.shape != (256,):
            raise ValueError("level_pos must be [3][256] and out_thresholds [256]")
        h = C.c_void_p()
        _check(self.L.gs360_color_plan_create(self.handle, lut.ctypes.data, int(lut.shape[0]), pos.ctypes.data,
                                              thr.ctypes.data, C.byref(h)), self.L)
        return h

    def color_plan_free(self, plan):
        if plan:
            _check(self.L.gs360_color_plan_destroy(self.handle, plan), self.L)

    def color_plan16(self, lut_table, domain_min, domain_max, n_pieces, start, base, off, thresholds):
        """16-bit colour plan (include/gs360.h): LUT + domain + the piecewise output thresholds of gs360.color.output_pieces16."""
        lut = self._color_lut(lut_table)
        dmin = np.ascontiguousarray(domain_min, dtype=np.float32)
        dmax = np.ascontiguousarray(domain_max, dtype=np.float32)
        st = np.ascontiguousarray(start, dtype=np.float32)
        ba = np.ascontiguousarray(base, dtype=np.int32)
        of = np.ascontiguousarray(off, dtype=np.int32)
        th = np.ascontiguousarray(thresholds, dtype=np.float32)
        if dmin.shape != (3,) or dmax.shape != (3,) or st.size < 4 or ba.size < 4 or of.size < 5:
            raise ValueError("bad colour plan tables")
        h = C.c_void_p()
        _check(self.L.gs360_color_plan16_create(self.handle, lut.ctypes.data, int(lut.shape[0]), dmin.ctypes.data, dmax.ctypes.data,
                                                int(n_pieces), st.ctypes.data, ba.ctypes.data, of.ctypes.data,
                                                th.ctypes.data if th.size else None, C.byref(h)), self.L)
        return h

    def color_plan16_free(self, plan):
        if plan:
            _check(self.L.gs360_color_plan16_destroy(self.handle, plan), self.L)

    def _color_apply(self, fn, plan, src, H, W, Cn, dst, red_index, src_stride, dst_stride, slot):
        _check(fn(self.handle, plan, src.ptr, H, W, Cn, src_stride, red_index, (dst or src).ptr, dst_stride, slot), self.L)

    def color_apply16_dev(self, plan, src, H, W, Cn, dst=None, red_index=0, src_stride=0, dst_stride=0, slot=0):
        self._color_apply(self.L.gs360_color_apply_u16, plan, src, H, W, Cn, dst, red_index, src_stride, dst_stride, slot)

    def color_apply_dev(self, plan, src, H, W, Cn, dst=None, red_index=0, src_stride=0, dst_stride=0, slot=0):
        """Apply a colour plan to a device-resident H x W x C image (in place when dst is None)."""
        self._color_apply(self.L.gs360_color_apply_u8, plan, src, H, W, Cn, dst, red_index, src_stride, dst_stride, slot)

    # -- decoded video frames to RGB (gs360/vidcolor.py) ---------------------------------------
    def video_plan(self, depth, full_range, keep_rec709, primaries, linear, encode, out_bits=None):
        """gs360_video_plan_create_out: primaries float32 [3][3], linear float32 [16384], encode float32 [1024][2] (gs360/vidcolor.py
        builds them); out_bits None = the depth's own pairing (8 -> 8, 10 -> 16), 8 with depth 10 = uint8 RGB from 10-bit planes.
        Returns an opaque plan handle (free with video_plan_free)."""
        if out_bits is None:
            out_bits = 8 if int(depth) == 8 else 16
        m = np.ascontiguousarray(primaries, dtype=np.float32)
        lin = np.ascontiguousarray(linear, dtype=np.float32)
        enc = np.ascontiguousarray(encode, dtype=np.float32)
        if m.shape != (3, 3) or lin.shape != (16384,) or enc.shape != (1024, 2):
            raise ValueError("primaries must be [3][3], linear [16384] and encode [1024][2]")
        h = C.c_void_p()
        _check(self.L.gs360_video_plan_create_out(self.handle, int(depth), int(out_bits), int(full_range), int(keep_rec709), m.ctypes.data,
                                                  lin.ctypes.data, enc.ctypes.data, C.byref(h)), self.L)
        return h

    def video_plan_free(self, plan):
        if plan:
            _check(self.L.gs360_video_plan_destroy(self.handle, plan), self.L)

    @staticmethod
    def _video_jobs(jobs):
        def addr(b):
            return b.ptr if isinstance(b, DeviceBuffer) else int(b)
        arr = (VideoJob * max(len(jobs), 1))()
        for k, (y, cb, cr, W, H, sub, dst, *strides) in enumerate(jobs):
            ys, cbs, crs, ds = (list(strides) + [0, 0, 0, 0])[:4]
            arr[k] = VideoJob(addr(y), addr(cb), addr(cr), int(ys), int(cbs), int(crs), int(W), int(H), int(sub), 0, addr(dst), int(ds))
        return arr

    def video_rgb_dev(self, plan, jobs, slot=0):
        """gs360_video_rgb: jobs = sequence of (y, cb, cr, W, H, subsampling, dst[, y_stride, cb_stride, cr_stride, dst_stride]),
        the planes and dst DeviceBuffers or device addresses, strides in bytes (0 = tight).  Asynchronous on `slot`."""
        _check(self.L.gs360_video_rgb(self.handle, plan, self._video_jobs(jobs), len(jobs), slot), self.L)

    def video_fisheye_rgb_dev(self, plan, view, jobs, slot=0):
        """gs360_video_fisheye_rgb: view = (projection, size, W, H, input_fov_deg, h_fov_deg, v_fov_deg) or None (a NULL view); jobs
        as for video_rgb_dev, every job's W x H the view's and its dst size x size x 3.  Asynchronous on `slot`."""
        v = None if view is None else C.byref(VideoFisheyeView(int(view[0]), int(view[1]), int(view[2]), int(view[3]),
                                                               float(view[4]), float(view[5]), float(view[6])))
        _check(self.L.gs360_video_fisheye_rgb(self.handle, plan, v, self._video_jobs(jobs), len(jobs), slot), self.L)

    # -- frame sharpness statistics (gs360/framescore.py) -------------------------------------
    def _by_depth(self, name, depth):
        """The _u8 or _u16 entry point of a FrameSelector pass (depth: bits per sample, 8 or 16)."""
        if depth not in (8, 16):
            raise ValueError(f"depth must be 8 or 16 (got {depth!r})")
        return getattr(self.L, f"{name}_u{depth}")

    def frame_stats_dev(self, frames, H, W, Cn, band, stats, flags=0, smalls=None, small_w=0, small_h=0, red_index=0, stride=0, slot=0,
                        depth=8):
        """gs360_frame_stats_u8 (depth 16: _u16) on device frames (list of DeviceBuffer, H x W x C uint8 / uint16): stats =
        DeviceBuffer of len(frames) FrameStats records; smalls = None or one DeviceBuffer of 2 x small_h x small_w float32 per
        frame.  band = (y0, y1).  Asynchronous on `slot`."""
        nf = len(frames)
        fp = (C.c_void_p * max(nf, 1))(*[b.ptr for b in frames])
        sp = (C.c_void_p * max(nf, 1))(*[b.ptr for b in smalls]) if smalls is not None else None
        fn = self._by_depth("gs360_frame_stats", depth)
        _check(fn(self.handle, fp, nf, int(H), int(W), int(Cn), int(stride), int(red_index), int(band[0]),
                  int(band[1]), int(flags), stats.ptr, sp, int(small_w), int(small_h), slot), self.L)

    def frame_edge_dev(self, frames, H, W, Cn, band, out, red_index=0, stride=0, slot=0, depth=8):
        """gs360_frame_edge_u8 (depth 16: _u16) on device frames (list of DeviceBuffer, H x W x C uint8 / uint16): out =
        DeviceBuffer of len(frames) FrameEdge records.  band = (y0, y1).  Asynchronous on `slot`."""
        nf = len(frames)
        fp = (C.c_void_p * max(nf, 1))(*[b.ptr for b in frames])
        fn = self._by_depth("gs360_frame_edge", depth)
        _check(fn(self.handle, fp, nf, int(H), int(W), int(Cn), int(stride), int(red_index), int(band[0]),
                  int(band[1]), out.ptr, slot), self.L)

    def frame_fft_energy_dev(self, smalls, small_w, small_h, H, W, band, out, flags=0, slot=0):
        """gs360_frame_fft_energy on the fft inputs frame_stats_dev wrote (one DeviceBuffer of 2 x small_h x small_w float32 per
        frame of H x W, band = (y0, y1)): out = DeviceBuffer of len(smalls) FrameFft records.  Asynchronous on `slot`."""
        nf = len(smalls)
        sp = (C.c_void_p * max(nf, 1))(*[b.ptr for b in smalls])
        _check(self.L.gs360_frame_fft_energy(self.handle, sp, nf, int(small_w), int(small_h), int(H), int(W), int(band[0]),
                                             int(band[1]), int(flags), out.ptr, slot), self.L)

    def frame_flow_dev(self, frames, H, W, Cn, crop, small_w, small_h, pairs, out, flags=0, points=None, red_index=0, stride=0, slot=0,
                       depth=8):
        """gs360_frame_flow_u8 (depth 16: _u16) on device frames (list of DeviceBuffer, H x W x C uint8 / uint16): crop = (x0, y0,
        w, h), pairs = sequence of (prev, curr) indices into frames; out = DeviceBuffer of len(pairs) FrameFlow records; points =
        None or a DeviceBuffer of len(pairs) x FLOW_MAX_CORNERS FlowPoint records.  Asynchronous on `slot`."""
        nf = len(frames)
        fp = (C.c_void_p * max(nf, 1))(*[b.ptr for b in frames])
        flat = [int(v) for pr in pairs for v in pr]
        pa = (C.c_int * max(len(flat), 1))(*flat)
        fn = self._by_depth("gs360_frame_flow", depth)
        _check(fn(self.handle, fp, nf, int(H), int(W), int(Cn), int(stride), int(red_index), int(crop[0]),
                  int(crop[1]), int(crop[2]), int(crop[3]), int(small_w), int(small_h), int(flags), pa,
                  len(pairs), out.ptr, points.ptr if points is not None else None, slot), self.L)

    # -- JPEG scans of device images (gs360/jpegenc.py) ---------------------------------------
    @staticmethod
    def _encoder_jobs(struct, jobs, fill):
        """The job array of an encoder call: the out_capacity check (a job ends with its out buffer and out_capacity) and
        fill(*job) -> the job's struct, per codec."""
        arr = (struct * max(len(jobs), 1))()
        for k, job in enumerate(jobs):
            if job[-1] > job[-2].nbytes:
                raise ValueError("out_capacity larger than the output buffer")
            arr[k] = fill(*job)
        return arr

    @staticmethod
    def _jpeg_job(src, H, W, Cn, stride, out, cap):
        return JpegJob(src.ptr, int(H), int(W), int(Cn), int(stride), out.ptr, int(cap))

    @staticmethod
    def _png_job(src, H, W, Cn, bps, stride, out, cap):
        return PngJob(src.ptr if isinstance(src, DeviceBuffer) else int(src), int(H), int(W), int(Cn), int(bps), int(stride), out.ptr, int(cap))

    def _jpeg_scan(self, fn, jobs, head, lengths, tables, slot):
        """What the three scan entry points share: the tables buffer's size check, the job array and the call.  head = (quality,
        restart[, subsampling]); tables = (DeviceBuffer or None,), or () for the entry point without the argument."""
        for t in tables:
            if t is not None and t.nbytes < 4 * JPEG_TABLE_BYTES * len(jobs):
                raise ValueError("tables buffer below 4 x 272 bytes per job")
        arr = self._encoder_jobs(JpegJob, jobs, self._jpeg_job)
        _check(fn(self.handle, arr, len(jobs), *(int(v) for v in head), lengths.ptr,
                  *(t.ptr if t is not None else None for t in tables), slot), self.L)

    def jpeg_scan_dev(self, jobs, lengths, quality=100, restart=8, slot=0):
        """gs360_jpeg_scan_u8: jobs = iterable of (src DeviceBuffer, H, W, C, src_stride, out DeviceBuffer, out_capacity); lengths =
        DeviceBuffer of len(jobs) uint64 (JPEG_OVERFLOW where a scan exceeded its capacity).  Asynchronous on `slot`."""
        self._jpeg_scan(self.L.gs360_jpeg_scan_u8, jobs, (quality, restart), lengths, (), slot)

    def jpeg_scan_opt_dev(self, jobs, lengths, tables, quality=100, restart=8, slot=0):
        """gs360_jpeg_scan_opt_u8: jpeg_scan_dev with every image's own optimal Huffman tables; tables = DeviceBuffer of
        len(jobs) * 4 * JPEG_TABLE_BYTES bytes (per image DC0, AC0, DC1, AC1).  Asynchronous on `slot`."""
        self._jpeg_scan(self.L.gs360_jpeg_scan_opt_u8, jobs, (quality, restart), lengths, (tables,), slot)

    def jpeg_scan_sub_dev(self, jobs, lengths, tables=None, quality=100, restart=8, subsampling=JPEG_444, slot=0):
        """gs360_jpeg_scan_sub_u8: jpeg_scan_dev (tables None: the Annex K tables) or jpeg_scan_opt_dev (tables = DeviceBuffer of
        len(jobs) * 4 * JPEG_TABLE_BYTES bytes) with the chroma subsampling JPEG_444 or JPEG_420.  Asynchronous on `slot`."""
        self._jpeg_scan(self.L.gs360_jpeg_scan_sub_u8, jobs, (quality, restart, subsampling), lengths, (tables,), slot)

    def jpeg_huff_tables_dev(self, hist, n, tables, slot=0):
        """gs360_jpeg_huff_tables: hist = DeviceBuffer of n * 256 uint32 symbol counts -> tables = DeviceBuffer of n * JPEG_TABLE_BYTES
        bytes (16 BITS + HUFFVAL, zero padded).  Asynchronous on `slot`."""
        if hist.nbytes < 1024 * n or tables.nbytes < JPEG_TABLE_BYTES * n:
            raise ValueError("histogram or tables buffer too small for n tables")
        _check(self.L.gs360_jpeg_huff_tables(self.handle, hist.ptr, int(n), tables.ptr, slot), self.L)

    # -- PNG deflate streams of device images (gs360/pngenc.py) -------------------------------
    def png_deflate_dev(self, jobs, lengths, adler, slot=0):
        """gs360_png_deflate: jobs = iterable of (src DeviceBuffer or device address, H, W, C, bytes_per_sample, src_stride, out
        DeviceBuffer, out_capacity); lengths = DeviceBuffer of len(jobs) uint64 (PNG_OVERFLOW where a stream exceeded its capacity);
        adler = DeviceBuffer of two uint32 per chunk of PNG_CHUNK filtered bytes, the jobs' chunks in job order.  Asynchronous on
        `slot`."""
        jobs = list(jobs)
        arr = self._encoder_jobs(PngJob, jobs, self._png_job)
        chunks = sum(-(-(int(H) * (1 + int(W) * int(Cn) * int(bps))) // PNG_CHUNK) for _src, H, W, Cn, bps, *_rest in jobs)
        if lengths.nbytes < 8 * len(jobs) or adler.nbytes < 8 * chunks:
            raise ValueError("lengths or adler buffer too small")
        _check(self.L.gs360_png_deflate(self.handle, arr, len(jobs), lengths.ptr, adler.ptr, slot), self.L)

    # -- segmentation masks finished on the device (gs360/maskfinish.py) -----------------------
    def mask_finish_scratch(self, jobs):
        """gs360_mask_finish_scratch: jobs = sequence of MaskJob -> the bytes of scratch one gs360_mask_finish_u8 call on them needs"""
        n = C.c_size_t(0)
        arr = (MaskJob * max(len(jobs), 1))(*jobs)
        _check(self.L.gs360_mask_finish_scratch(arr, len(jobs), C.byref(n)), self.L)
        return int(n.value)

    def mask_finish_dev(self, jobs, scratch, counts, slot=0, scratch_bytes=None):
        """gs360_mask_finish_u8: jobs = sequence of MaskJob (gs360/maskfinish.py fills them), scratch = DeviceBuffer of
        mask_finish_scratch(jobs) bytes, counts = DeviceBuffer of len(jobs) uint32.  The kernels are asynchronous on `slot`."""
        if counts.nbytes < 4 * len(jobs):
            raise ValueError("counts buffer below 4 bytes per job")
        nbytes = scratch.nbytes if scratch_bytes is None else int(scratch_bytes)
        if nbytes > scratch.nbytes:
            raise ValueError("scratch_bytes larger than the scratch buffer")
        arr = (MaskJob * max(len(jobs), 1))(*jobs)
        _check(self.L.gs360_mask_finish_u8(self.handle, arr, len(jobs), scratch.ptr, nbytes, counts.ptr, slot), self.L)

    def mask_shadow_scratch(self, jobs):
        """gs360_mask_shadow_scratch: jobs = sequence of ShadowJob -> the bytes of scratch the two shadow calls on them share"""
        n = C.c_size_t(0)
        arr = (ShadowJob * max(len(jobs), 1))(*jobs)
        _check(self.L.gs360_mask_shadow_scratch(arr, len(jobs), C.byref(n)), self.L)
        return int(n.value)

    def _mask_shadow_call(self, fn, jobs, scratch, counts, slot, scratch_bytes):
        if counts.nbytes < 4 * len(jobs):
            raise ValueError("counts buffer below 4 bytes per job")
        nbytes = scratch.nbytes if scratch_bytes is None else int(scratch_bytes)
        if nbytes > scratch.nbytes:
            raise ValueError("scratch_bytes larger than the scratch buffer")
        arr = (ShadowJob * max(len(jobs), 1))(*jobs)
        _check(fn(self.handle, arr, len(jobs), scratch.ptr, nbytes, counts.ptr, slot), self.L)

    def mask_shadow_candidates_dev(self, jobs, scratch, counts, slot=0, scratch_bytes=None):
        """gs360_mask_shadow_candidates_u8: leaves P and C0 in `scratch` and count(P) per job in `counts` (DeviceBuffers);
        asynchronous on `slot`"""
        self._mask_shadow_call(self.L.gs360_mask_shadow_candidates_u8, jobs, scratch, counts, slot, scratch_bytes)

    def mask_shadow_merge_dev(self, jobs, scratch, counts, slot=0, scratch_bytes=None):
        """gs360_mask_shadow_merge_u8 on the scratch the candidates call left: M into every job's dst, count(M) into `counts`;
        returns when the kernels are done"""
        self._mask_shadow_call(self.L.gs360_mask_shadow_merge_u8, jobs, scratch, counts, slot, scratch_bytes)

    def mask_inpaint_scratch(self, jobs):
        """gs360_mask_inpaint_scratch: jobs = sequence of InpaintJob -> the bytes of scratch one gs360_mask_inpaint_u8 call on them needs"""
        n = C.c_size_t(0)
        arr = (InpaintJob * max(len(jobs), 1))(*jobs)
        _check(self.L.gs360_mask_inpaint_scratch(arr, len(jobs), C.byref(n)), self.L)
        return int(n.value)

    def mask_inpaint_dev(self, jobs, scratch, levels, slot=0, scratch_bytes=None):
        """gs360_mask_inpaint_u8: jobs = sequence of InpaintJob whose images are filled in place, scratch = DeviceBuffer of
        mask_inpaint_scratch(jobs) bytes, levels = DeviceBuffer of len(jobs) uint32 (K per job).  Returns when the kernels are done."""
        if levels.nbytes < 4 * len(jobs):
            raise ValueError("levels buffer below 4 bytes per job")
        nbytes = scratch.nbytes if scratch_bytes is None else int(scratch_bytes)
        if nbytes > scratch.nbytes:
            raise ValueError("scratch_bytes larger than the scratch buffer")
        arr = (InpaintJob * max(len(jobs), 1))(*jobs)
        _check(self.L.gs360_mask_inpaint_u8(self.handle, arr, len(jobs), scratch.ptr, nbytes, levels.ptr, slot), self.L)

    # -- JPEG files decoded into device images (gs360/jpegdec.py) ------------------------------
    # -- voxel downsampling of a resident point cloud (gs360/pointcloud.py) -----------------------
    def voxel_scratch(self, n):
        """gs360_voxel_scratch: the bytes of scratch the bounds, count and pick calls on a cloud of n points share"""
        nbytes = C.c_size_t(0)
        _check(self.L.gs360_voxel_scratch(self.handle, int(n), C.byref(nbytes)), self.L)
        return int(nbytes.value)

    def cloud_bounds_dev(self, xyz, n, scratch, slot=0):
        """gs360_cloud_bounds_f32: xyz = DeviceBuffer of n x 3 float32 -> float32[6], the per-axis minimum then maximum"""
        out = (C.c_float * 6)()
        _check(self.L.gs360_cloud_bounds_f32(self.handle, xyz.ptr, int(n), scratch.ptr, scratch.nbytes, out, slot), self.L)
        return np.array(out, dtype=np.float32)

    def voxel_count_dev(self, xyz, n, minmax, voxel, scratch, slot=0):
        """gs360_voxel_count_f32: the number of occupied voxels of edge float32(voxel) on the grid at minmax[:3]"""
        mm = (C.c_float * 6)(*[float(v) for v in minmax])
        count = C.c_int64(0)
        _check(self.L.gs360_voxel_count_f32(self.handle, xyz.ptr, int(n), mm, float(voxel), scratch.ptr, scratch.nbytes, C.byref(count), slot),
               self.L)
        return int(count.value)

    def voxel_pick_dev(self, xyz, n, minmax, voxel, strategy, scratch, pick=None, order=None, starts=None, slot=0):
        """gs360_voxel_pick_f32 -> k; pick / order / starts = DeviceBuffers of n uint32 (or None) that receive the representatives, the
        indices in stable key order and the segment starts"""
        mm = (C.c_float * 6)(*[float(v) for v in minmax])
        k = C.c_int64(0)
        ptr = [b.ptr if b is not None else None for b in (pick, order, starts)]
        _check(self.L.gs360_voxel_pick_f32(self.handle, xyz.ptr, int(n), mm, float(voxel), int(strategy), scratch.ptr, scratch.nbytes,
                                           ptr[0], ptr[1], ptr[2], C.byref(k), slot), self.L)
        return int(k.value)

    # -- adaptive octree sampling of a resident point cloud (gs360/pointcloud.py) -----------------
    def octree_scratch(self, n):
        """gs360_octree_scratch: the bytes of scratch gs360_octree_pick_f32 needs for a cloud of n points"""
        nbytes = C.c_size_t(0)
        _check(self.L.gs360_octree_scratch(self.handle, int(n), C.byref(nbytes)), self.L)
        return int(nbytes.value)

    def octree_pick_dev(self, xyz, n, cube_min, cube_size, target, weight_power, min_voxel, strategy, scratch, order=None, slot=0, stages=False):
        """gs360_octree_pick_f32 -> (picks, starts, counts, stage_ms): uint32 arrays of the k kept leaves in output order (picks is None
        with VOXEL_SEGMENTS, starts and counts are None without it; they index `order`, a DeviceBuffer of n uint32), and the nine
        stage times in milliseconds when `stages` is set"""
        corner = (C.c_float * 3)(*[float(v) for v in cube_min])
        k = C.c_int64(0)
        segments = strategy == VOXEL_SEGMENTS
        pick = None if segments else np.empty(int(target), dtype=np.uint32)
        starts, counts = (np.empty(int(target), dtype=np.uint32), np.empty(int(target), dtype=np.uint32)) if segments else (None, None)
        ms = (C.c_double * 9)() if stages else None
        ptr = [a.ctypes.data if a is not None else None for a in (pick, starts, counts)]
        _check(self.L.gs360_octree_pick_f32(self.handle, xyz.ptr, int(n), corner, float(cube_size), int(target), float(weight_power), float(min_voxel),
                                            int(strategy), scratch.ptr, scratch.nbytes, ptr[0], order.ptr if order is not None else None, ptr[1],
                                            ptr[2], C.byref(k), ms, slot), self.L)
        k = int(k.value)
        return tuple(a[:k] if a is not None else None for a in (pick, starts, counts)) + (list(ms) if stages else None,)

    def jpeg_decode_dev(self, jobs, status, slot=0):
        """gs360_jpeg_decode_u8: jobs = sequence of JpegDecJob (device pointers; gs360/jpegdec.py fills them), status = DeviceBuffer of
        len(jobs) uint32.  Asynchronous on `slot`."""
        if status.nbytes < 4 * len(jobs):
            raise ValueError("status buffer below 4 bytes per job")
        arr = (JpegDecJob * max(len(jobs), 1))(*jobs)
        _check(self.L.gs360_jpeg_decode_u8(self.handle, arr, len(jobs), status.ptr, slot), self.L)

    def jpeg_decode_gray_dev(self, jobs, status, slot=0):
        """gs360_jpeg_decode_gray_u8: as jpeg_decode_dev, but every job's `out` is an H x W plane of FS-SPEC's gray (out_stride 0 or at
        least W).  Asynchronous on `slot`."""
        if status.nbytes < 4 * len(jobs):
            raise ValueError("status buffer below 4 bytes per job")
        arr = (JpegDecJob * max(len(jobs), 1))(*jobs)
        _check(self.L.gs360_jpeg_decode_gray_u8(self.handle, arr, len(jobs), status.ptr, slot), self.L)

    # -- hot path, host buffers (synchronous) -----------------------------------------------
    def equirect_views(self, src, views, slot=0, interp=INTERP_LINEAR, flags=0):
        """src: H x W x C uint8 (or uint16) ndarray -> list of per-view ndarrays (height x width x C) of the same dtype."""
        dt = np.uint16 if np.asarray(src).dtype == np.uint16 else np.uint8
        src = np.ascontiguousarray(src, dtype=dt)
        if src.ndim == 2:
            src = src[:, :, None]
        H, W, Cn = src.shape
        outs = [np.empty((v.height, v.width, Cn), dt) for v in views]
        if not views:
            return outs
        va = (View * len(views))(*views)
        dp = (C.c_void_p * len(views))(*[o.ctypes.data for o in outs])
        with self.slot_locks[slot]:
            fn = self.L.gs360_equirect_views_u16_host if dt == np.uint16 else self.L.gs360_equirect_views_u8_host
            _check(fn(self.handle, src.ctypes.data, W, H, Cn, src.strides[0], va, len(views), dp, 0, interp, int(flags), slot), self.L)
        return outs

    def remap(self, src, map_x, map_y, interpolation=INTERP_LINEAR, border_value=0.0, valid=None, fill_value=0,
              slot=0):
        """cv2.remap(src, map_x, map_y, interpolation, borderMode=BORDER_CONSTANT, borderValue=...) drop-in
        (DF:2001-2008); `valid`/`fill_value` fuse the reference's `out[~valid] = mask_value` (DF:2009-2014).
        uint16 sources take cv2's CV_16U (float-weight) samplers and return uint16."""
        dt = np.uint16 if np.asarray(src).dtype == np.uint16 else np.uint8
        src = np.ascontiguousarray(src, dtype=dt)
        s3 = src if src.ndim == 3 else src[:, :, None]
        H, W, Cn = s3.shape
        mx = np.ascontiguousarray(map_x, dtype=np.float32)
        my = np.ascontiguousarray(map_y, dtype=np.float32)
        if mx.shape != my.shape or mx.ndim != 2:
            raise ValueError("map_x / map_y must be 2-D arrays of equal shape")
        h, w = mx.shape
        if np.isscalar(border_value):
            border_value = (float(border_value), 0.0, 0.0, 0.0)  # cv::Scalar(v)
        bv = (C.c_double * 4)(*[float(b) for b in (list(border_value) + [0, 0, 0, 0])[:4]])
        va = None
        if valid is not None:
            va = np.ascontiguousarray(valid, dtype=np.uint8)
            if va.shape != (h, w):
                raise ValueError("valid mask shape mismatch")
        dst = np.empty((h, w, Cn), dt)
        with self.slot_locks[slot]:
            fn = self.L.gs360_remap_table_u16_host if dt == np.uint16 else self.L.gs360_remap_table_u8_host
            _check(fn(self.handle, s3.ctypes.data, H, W, Cn, s3.strides[0], mx.ctypes.data, my.ctypes.data,
                      va.ctypes.data if va is not None else None, h, w, int(interpolation), bv, int(fill_value), dst.ctypes.data, 0, slot),
                   self.L)
        return dst if src.ndim == 3 else dst[:, :, 0]
