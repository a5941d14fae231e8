"""Frame sharpness scoring on the GPU: the per-frame pass of the FrameSelector tool (FS-SPEC v1).

Drop-in seams of cli_tools/gs360_FrameSelector.py:
  score_one_file(fp, metric, crop_ratio, max_long, augment_motion, ignore_highlights, mask_mode="none")   FS:902-1044
  score_one_record(record, metric, crop_ratio, max_long, augment_motion, ignore_highlights, score_backend) FS:458-517
  score_one_file_ffmpeg(fp, metric, crop_ratio, max_long, augment_motion, ignore_highlights, mask_mode="none") FS:826-899
all return the reference's 9-tuple (sharp, p0, p255, brightness_mean, brightness_weight, lap_feature, ten_feature, fft_feature,
motion_factor).  The per-pixel work (gray, masks, Laplacian, Sobel, the INTER_AREA downscale of fft_energy_fast) runs in
gs360_frame_stats_u8; what is left here is the reference's branch logic on exact integer sums, in double, and the FFT of the
<= 512-pixel image (FS:742-786).  That FFT runs on the host (fft="host": NumPy, the reference's own code, on the downloaded
planes) or on the device (fft="device": gs360_frame_fft_energy, FS-FFT v1, after the statistics on the same stream; only two small
records per frame come back).  The reference's default backend ("ffmpeg": a filter graph's two YAVG values, whatever the metric)
is gs360_frame_edge_u8 (FS-EDGE v1) with the branch logic of FS:875-896 here; no ffmpeg is spawned.  score_arrays / edge_arrays /
score_files batch frames GS360_MAX_FRAMES per launch; hybrid_scores is the main
flow's per-run normalisation of the hybrid features (FS:2363-2392).

The path-based seams decode with imageio (Pillow) on the host; with GS360_JPEG_DECODER=device they read through
gs360/framesource.py instead, which decodes baseline JPEG files on the GPU into gray planes (DeviceFrames with C = 1).

8-bit sources by default: 16-bit and float images raise Gs360Error (GS360_ERR_UNSUPPORTED), as does max_long > 0.  With
GS360_FS_DEPTH16=device (FS-DEPTH16 v1) uint16 frames, the 16-bit PNG / TIFF frames Video2Frames writes for
sources of more than 8 bits per sample, go through gs360_frame_stats_u16 (exact sums on the 16-bit gray, in units of 1/257 gray
level; finish(unit=257)) and gs360_frame_edge_u16 (the edge pass on the samples' high bytes).  Float images stay refused.
"""
import collections
import concurrent.futures
import contextlib
import math
import os
import threading

import numpy as np

from . import capi, imageio, jpegdec

HYBRID_LAPVAR_WEIGHT = 0.6        # FS:311-315 (the code's weights; the docstring's 0.2 is not what runs)
HYBRID_TENENGRAD_WEIGHT = 0.3
HYBRID_FFT_WEIGHT = 0.1
HYBRID_MOTION_REFERENCE = 5000.0
HYBRID_MOTION_PENALTY_WEIGHT = 0.4
HYBRID_DARK_THRESHOLD = 0.35      # FS:330-331
HYBRID_DARK_PENALTY_WEIGHT = 0.5
FFT_LONG_SIDE = 512               # fft_energy_fast's downscale target (FS:754)
HIGHLIGHT_LEVEL = 243             # gray >= 0.95 * 255 = 242.25 on integer gray (FS:945)
METRICS = ("lapvar", "tenengrad", "fft", "hybrid")
FAILED = (None, 0.0, 0.0, 0.0, 1.0, None, None, None, 1.0)   # the reference's tuple for an unreadable image
FIELDS = tuple(n for n, _ in capi.FrameStats._fields_)
FFT_MODES = ("host", "device")
DEFAULT_FFT = "host"              # where score_* compute the fft term when their `fft` keyword is None
FFT_DTYPE = capi.record_dtype(capi.FrameFft)
EDGE_FIELDS = tuple(n for n, _ in capi.FrameEdge._fields_)

HIGHLIGHT_LEVEL16 = 62259        # FS-DEPTH16 v1: the smallest 16-bit gray g16 with g16 / 257 >= 242.25
UNIT16 = 257                      # a 16-bit frame's sums are in units of 1 / 257 gray level (255 / 65535 = 1 / 257)

# An H x W x C frame already in device memory, of uint8 samples or (depth 16) uint16 ones in host byte order.  stride: bytes from
# one row to the next, 0 = packed rows (W * C samples).  Every frame keeps its own: frames of one shape and different strides never
# share a launch (the C entry points take one stride per call).
DeviceFrame = collections.namedtuple("DeviceFrame", "buf H W C stride depth")
DeviceFrame.__new__.__defaults__ = (0, 8)


def depth16_mode_from_env():
    """-> True when 16-bit frames are scored and tracked on the GPU (FS-DEPTH16 v1).  GS360_FS_DEPTH16 = off (default: they are
    refused as before) | device; any other value is a ValueError."""
    mode = os.environ.get("GS360_FS_DEPTH16", "off")
    if mode not in ("off", "device"):
        raise ValueError(f"GS360_FS_DEPTH16 must be off or device (got {mode!r})")
    return mode == "device"


def band_rows(H, crop_ratio):
    """crop_by_ratio_gray_and_mask's band (FS:674-690) -> (y0, y1); ValueError outside (0, 1]."""
    if crop_ratio is None or abs(crop_ratio - 1.0) < 1e-6:
        return 0, H
    if not (0.0 < crop_ratio <= 1.0):
        raise ValueError("crop_ratio must be in (0, 1]")
    nh = max(1, int(H * crop_ratio))
    y0 = max(0, (H - nh) // 2)
    return y0, min(H, y0 + nh)


def edge_band_rows(H, crop_ratio):
    """The filter graph's crop (FS:796-800) -> (y0, y1): only when crop_ratio < 1.0, height max(1, trunc(H * crop_ratio)) at
    trunc((H - height) / 2)."""
    if crop_ratio is None or not crop_ratio < 1.0:
        return 0, H
    bh = max(1, math.trunc(H * crop_ratio))
    y0 = math.trunc((H - bh) / 2)
    return y0, y0 + bh


def yavg(total, n):
    """signalstats' YAVG as the reference reads it (FS:813-823): the mean printed with %g, six significant digits, parsed back."""
    return float("%g" % (total / n))


def finish_edge(rec):
    """The 9-tuple of score_one_file_ffmpeg (FS:875-896) from one frame's gs360_frame_edge record (mapping of its fields)."""
    brightness_mean = max(0.0, min(1.0, yavg(rec["sum_gray"], rec["n"]) / 255.0))
    sharp = max(0.0, min(1.0, yavg(rec["sum_edge"], rec["n"]) / 255.0))
    dark_ratio = brightness_mean / HYBRID_DARK_THRESHOLD if brightness_mean < HYBRID_DARK_THRESHOLD else 1.0
    dark_ratio = max(0.0, min(1.0, dark_ratio))
    brightness_weight = max(0.0, 1.0 - HYBRID_DARK_PENALTY_WEIGHT * (1.0 - dark_ratio))
    return (sharp, 0.0, 0.0, brightness_mean, brightness_weight, None, None, None, 1.0)


def fft_input_size(bw, bh):
    """(width, height) of the image fft_energy_fast transforms for a bw x bh band (FS:754-760): the band itself up to 512."""
    if max(bh, bw) > FFT_LONG_SIDE:
        scale = float(FFT_LONG_SIDE) / float(max(bh, bw))
        return max(1, int(bw * scale)), max(1, int(bh * scale))
    return bw, bh


def nearest_index(dsize, ssize):
    """cv2.resize INTER_NEAREST's source index per destination index: min(floor(d * (1 / (dsize / ssize))), ssize - 1)."""
    ifx = 1.0 / (float(dsize) / float(ssize))
    return np.minimum(np.floor(np.arange(dsize) * ifx).astype(np.int64), ssize - 1)


def circle_mask(H, W, ys, xs):
    """build_circular_valid_mask (FS:693-705) at rows ys x columns xs of an H x W frame, in integers."""
    r4 = max(4, min(W, H) ** 2)
    dy = 2 * np.asarray(ys, np.int64)[:, None] - (H - 1)
    dx = 2 * np.asarray(xs, np.int64)[None, :] - (W - 1)
    return dx * dx + dy * dy <= r4


def fft_energy(g, g_mask):
    """fft_energy_fast after its resize (FS:762-786), on the float32 image g and the resized mask (or None)."""
    f = np.fft.fft2(g.astype(np.float32))
    fshift = np.fft.fftshift(f)
    h, w = g.shape
    cy, cx = h // 2, w // 2
    r = max(1, min(h, w) // 8)
    yy, xx = np.ogrid[:h, :w]
    dist2 = (yy - cy) ** 2 + (xx - cx) ** 2
    hf_abs = np.abs(fshift * (dist2 >= r * r).astype(np.float32))
    if g_mask is not None and np.any(g_mask):
        valid = (g_mask > 0).astype(np.float32)
        total = np.sum(valid)
        if total > 0:
            return float(np.sum(hf_abs * valid) / total)
    return float(np.mean(hf_abs))


def fft_mode(fft):
    """The `fft` keyword of the score_* functions: None -> DEFAULT_FFT; "host" or "device"; anything else is a ValueError."""
    mode = DEFAULT_FFT if fft is None else fft
    if mode not in FFT_MODES:
        raise ValueError(f"fft must be one of {FFT_MODES} or None (got {fft!r})")
    return mode


def fft_energy_from_record(rec, masked):
    """fft_energy's value from a gs360_frame_fft record (mapping of its fields), with the reference's branches (FS:779-786): the
    valid mean when a mask exists and is not empty, else the mean over all h*w positions."""
    if masked and rec["n_valid"] > 0:
        return float(rec["sum_hf_valid"] / float(rec["n_valid"]))
    return float(rec["sum_hf"] / float(rec["n"]))


def _cv_mean(s, n):
    return s * (1.0 / n)          # cv::mean: sum * (1. / count)


def _cv_var(s, sq, n):
    """std^2 of cv::meanStdDev: mean = s * (1/n), std = sqrt(max(sq * (1/n) - mean^2, 0))."""
    scale = 1.0 / n
    m = s * scale
    std = math.sqrt(max(sq * scale - m * m, 0.0))
    return std * std


def mask_plan(st, H, W, ignore_highlights, mask_mode):
    """-> (p255, masked): the reference's mask branches (FS:938-961) decided from the full-frame counts.  masked = the band
    statistics come from the valid sums (a mask exists; the empty-mask fallback is the caller's)."""
    circle = mask_mode == "fisheye_circle"
    p255 = 0.0
    masked = circle
    if ignore_highlights:
        if circle and st["n_circle"] > 0:
            p255 = float(st["n_highlight_in_circle"] / float(st["n_circle"]))
        else:
            p255 = float(st["n_highlight"] / float(H * W))
        if not circle:
            masked = 0.0 < p255 < 1.0
    return p255, masked


def in_gray_levels(st, unit):
    """A record whose sums are in units of 1 / unit gray level (gs360_frame_stats_u16: unit 257) with those sums in gray levels:
    sum_gray and sum_lap divided by unit, sum_lap2 and sum_mag2 by unit ** 2, each one correctly rounded integer division into a
    double.  The counts stay integers."""
    out = dict(st)
    for sfx in ("", "_valid"):
        for name, div in (("sum_gray", unit), ("sum_lap", unit), ("sum_lap2", unit * unit), ("sum_mag2", unit * unit)):
            out[name + sfx] = int(st[name + sfx]) / div
    return out


def finish(st, H, W, band, metric, augment_motion, ignore_highlights, mask_mode, small=None, fft_rec=None, unit=1):
    """The 9-tuple of score_one_file from one frame's statistics.  st: mapping of the gs360_frame_stats fields; small: the two
    planes of the fft input (INTER_AREA image, gray at the nearest sample) for metric fft / hybrid; fft_rec: instead of small, the
    frame's gs360_frame_fft record (mapping of its fields), computed with the flags of mask_mode and ignore_highlights.  unit: 1
    for an 8-bit frame's record, 257 for a 16-bit frame's (FS-DEPTH16 v1: the reference's float32 chain on g16 * 255 / 65535 with
    the rounding removed)."""
    if metric not in METRICS:
        return FAILED                 # the reference's `sharp` is never bound: its except clause returns this
    if unit != 1:
        st = in_gray_levels(st, unit)
    p255, masked = mask_plan(st, H, W, ignore_highlights, mask_mode)
    use_valid = masked and st["n_valid"] > 0
    sfx = "_valid" if use_valid else ""
    n = st["n_valid"] if use_valid else st["n"]
    if use_valid:
        brightness_mean = float(_cv_mean(float(st["sum_gray_valid"]), n) / 255.0)
    else:
        brightness_mean = float(st["sum_gray"] / n / 255.0)   # exact sum / n (the reference's np.mean sums in float32)
    brightness_weight = 1.0
    lap_feature = ten_feature = fft_feature = None
    motion_factor = 1.0
    lap = _cv_var(float(st["sum_lap" + sfx]), float(st["sum_lap2" + sfx]), n) if metric in ("lapvar", "hybrid") else None
    ten = _cv_mean(float(st["sum_mag2" + sfx]), n) if metric in ("tenengrad", "hybrid") else None
    fft = None
    if metric in ("fft", "hybrid") and fft_rec is not None:
        fft = fft_energy_from_record(fft_rec, masked)
    elif metric in ("fft", "hybrid"):
        g, g_near = small
        g_mask = None
        if masked:
            y0, y1 = band
            ys = y0 + nearest_index(g.shape[0], y1 - y0)
            xs = nearest_index(g.shape[1], W)
            m = np.ones(g.shape, bool)
            if mask_mode == "fisheye_circle":
                m &= circle_mask(H, W, ys, xs)
            if ignore_highlights:
                m &= g_near < HIGHLIGHT_LEVEL
            g_mask = m.astype(np.uint8)
        fft = fft_energy(g, g_mask)
    if metric == "lapvar":
        sharp = lap
        lap_feature = lap * lap
    elif metric == "tenengrad":
        sharp = ten_feature = ten
    elif metric == "fft":
        sharp = fft_feature = fft
    else:
        lap_feature, ten_feature, fft_feature = lap * lap, ten, fft
        hybrid_raw = HYBRID_LAPVAR_WEIGHT * lap_feature + HYBRID_TENENGRAD_WEIGHT * ten + HYBRID_FFT_WEIGHT * fft
        if augment_motion:
            motion_ratio = max(0.0, min(1.0, ten / (ten + HYBRID_MOTION_REFERENCE)))
            motion_factor = max(0.0, 1.0 - HYBRID_MOTION_PENALTY_WEIGHT * (1.0 - motion_ratio))
        dark_ratio = brightness_mean / HYBRID_DARK_THRESHOLD if brightness_mean < HYBRID_DARK_THRESHOLD else 1.0
        dark_ratio = max(0.0, min(1.0, dark_ratio))
        brightness_weight = max(0.0, 1.0 - HYBRID_DARK_PENALTY_WEIGHT * (1.0 - dark_ratio))
        sharp = hybrid_raw * motion_factor
    return (sharp, 0.0, p255, brightness_mean, brightness_weight, lap_feature, ten_feature, fft_feature, motion_factor)


def hybrid_scores(tuples):
    """The main flow's hybrid normalisation (FS:2363-2392): each feature min-max normalised over the run, blended with the hybrid
    weights and multiplied by the motion factor.  tuples: the run's 9-tuples; returns the final score column (a frame without a
    Laplacian feature keeps its own sharp value)."""
    lap_arr = [t[5] for t in tuples]
    ten_arr = [t[6] for t in tuples]
    fft_arr = [t[7] for t in tuples]
    lap_values = [v for v in lap_arr if v is not None]
    ten_values = [v for v in ten_arr if v is not None]
    fft_values = [v for v in fft_arr if v is not None]

    def _normalize(values, value):
        if not values or value is None:
            return 0.0
        vmin, vmax = min(values), max(values)
        if math.isclose(vmax, vmin):
            return 0.0
        return (value - vmin) / (vmax - vmin)

    scores = [t[0] for t in tuples]
    for i, t in enumerate(tuples):
        if lap_arr[i] is None:
            continue
        combined = (HYBRID_LAPVAR_WEIGHT * _normalize(lap_values, lap_arr[i]) + HYBRID_TENENGRAD_WEIGHT * _normalize(ten_values, ten_arr[i])
                    + HYBRID_FFT_WEIGHT * _normalize(fft_values, fft_arr[i]))
        scores[i] = combined * t[8]
    return scores


def mean_finite(values, default=None):
    """The mean of the values that are not None and finite; default when there is none."""
    valid = [float(v) for v in values if v is not None and math.isfinite(float(v))]
    if not valid:
        return default
    return float(sum(valid) / float(len(valid)))


# ---- the GPU pass ------------------------------------------------------------------------------------------------------------
_ctx = None
_ctx_lock = threading.Lock()


def default_context():
    """One engine context per process (device 0), created on first use."""
    global _ctx
    with _ctx_lock:
        if _ctx is None:
            _ctx = capi.Context(device=0, n_slots=1)
        return _ctx


def frame_shape(fr):
    """(H, W, C) of a DeviceFrame or a uint8 ndarray, with GS360_FS_DEPTH16=device also of a uint16 ndarray; Gs360Error
    (GS360_ERR_UNSUPPORTED) for other dtypes, ValueError for other shapes or another value of the variable."""
    if isinstance(fr, DeviceFrame):
        if fr.depth not in (8, 16):
            raise ValueError(f"DeviceFrame of depth {fr.depth!r}: want 8 or 16")
        if fr.depth == 16 and not depth16_mode_from_env():
            raise capi.Gs360Error(-4, "frame scoring takes 8-bit images (got a 16-bit DeviceFrame; 16-bit ones with GS360_FS_DEPTH16=device)")
        return fr.H, fr.W, fr.C
    a = np.asarray(fr)
    if a.dtype != np.uint8 and not (a.dtype == np.uint16 and depth16_mode_from_env()):
        raise capi.Gs360Error(-4, f"frame scoring takes 8-bit images (got {a.dtype}); 16-bit and float sources are not implemented"
                                  + (" (16-bit ones with GS360_FS_DEPTH16=device)" if a.dtype == np.uint16 else ""))
    if a.ndim == 2:
        return a.shape[0], a.shape[1], 1
    if a.ndim != 3 or a.shape[2] not in (1, 3, 4):
        raise ValueError(f"frame of shape {a.shape}: want H x W or H x W x C with C in (1, 3, 4)")
    return a.shape


def frame_depth(fr):
    """Bits per sample of a frame that frame_shape accepts: a DeviceFrame's depth, 16 for a uint16 ndarray, else 8."""
    if isinstance(fr, DeviceFrame):
        return fr.depth
    return 16 if np.asarray(fr).dtype == np.uint16 else 8


def depth_keyword(depth):
    """The `depth` keyword of Context.frame_stats_dev / frame_edge_dev / frame_flow_dev: named only for 16-bit frames, so that
    an 8-bit call is the call it was before the keyword existed."""
    return {"depth": 16} if depth == 16 else {}


def row_stride(fr):
    """A frame's row stride in bytes, normalised: a DeviceFrame's own (its 0 = packed rows, W * C samples), a host frame's packed
    row (host frames are uploaded contiguous)."""
    H, W, Cn = frame_shape(fr)
    packed = W * Cn * (frame_depth(fr) // 8)
    return (int(fr.stride) or packed) if isinstance(fr, DeviceFrame) else packed


def host_copy(ctx, fr):
    """A DeviceFrame's pixels as a packed H x W x C host ndarray (uint8, or uint16 at depth 16): one download of its rows, the
    padding dropped."""
    H, W, Cn = frame_shape(fr)
    stride = row_stride(fr)
    row = W * Cn * (fr.depth // 8)
    with ctx.slot_locks[0]:
        flat = ctx.download(fr.buf, ((H - 1) * stride + row,), np.uint8)
    rows = np.ascontiguousarray(np.lib.stride_tricks.as_strided(flat, (H, row), (stride, 1)))
    return rows.view(np.uint16 if fr.depth == 16 else np.uint8).reshape(H, W, Cn)


@contextlib.contextmanager
def device_frames(ctx, frames):
    """Device buffers of one launch's frames: a DeviceFrame's own buffer, a host frame uploaded.  Yields (bufs, stride, alloc):
    stride is the row stride all the frames share (0 = packed rows), alloc(nbytes) allocates an output buffer.  Frames of different
    row strides cannot share a launch: ValueError before anything is uploaded.  Whatever was uploaded or allocated is freed on
    exit."""
    owned = []

    def alloc(nbytes):
        owned.append(ctx.alloc(nbytes))
        return owned[-1]
    try:
        strides = {row_stride(fr) for fr in frames}
        if len(strides) > 1:
            raise ValueError(f"frames of row strides {sorted(strides)} in one launch: group them by stride")
        if len({frame_depth(fr) for fr in frames}) > 1:
            raise ValueError("8-bit and 16-bit frames in one launch: group them by sample type")
        bufs, stride = [], 0
        for fr in frames:
            if isinstance(fr, DeviceFrame):
                bufs.append(fr.buf)
                stride = 0 if row_stride(fr) == fr.W * fr.C * (fr.depth // 8) else row_stride(fr)
            else:
                owned.append(ctx.to_device(np.ascontiguousarray(fr)))
                bufs.append(owned[-1])
        yield bufs, stride, alloc
    finally:
        for b in owned:
            ctx.free(b)


def _batches(frames, shapes):
    """(i, j) index ranges of one launch each: consecutive frames of one size, one kind, one sample type and one row stride,
    GS360_MAX_FRAMES at most."""
    kinds = [(shape, isinstance(fr, DeviceFrame), frame_depth(fr), row_stride(fr)) for fr, shape in zip(frames, shapes)]
    i = 0
    while i < len(frames):
        j = i + 1
        while j < len(frames) and j - i < capi.MAX_FRAMES and kinds[j] == kinds[i]:
            j += 1
        yield i, j
        i = j


def _score_batch(ctx, frames, shape, metric, crop_ratio, augment_motion, ignore_highlights, mask_mode, red_index, fft):
    H, W, Cn = shape
    band = band_rows(H, crop_ratio)
    n = len(frames)
    depth = frame_depth(frames[0])            # one per batch (_batches)
    want_small = metric in ("fft", "hybrid")
    on_device = want_small and fft == "device"
    sw, sh = fft_input_size(W, band[1] - band[0])
    flags = (capi.FS_CIRCLE if mask_mode == "fisheye_circle" else 0) | (capi.FS_HIGHLIGHTS if ignore_highlights else 0)
    with device_frames(ctx, frames) as (bufs, stride, alloc):
        stats = alloc(n * capi.C.sizeof(capi.FrameStats))
        smalls = [alloc(2 * sw * sh * 4) for _ in range(n)] if want_small else None
        ffts = alloc(n * FFT_DTYPE.itemsize) if on_device else None
        with ctx.slot_locks[0]:
            ctx.frame_stats_dev(bufs, H, W, Cn, band, stats, flags=flags, smalls=smalls, small_w=sw, small_h=sh, red_index=red_index,
                                stride=stride, slot=0, **depth_keyword(depth))
            if on_device:
                ctx.frame_fft_energy_dev(smalls, sw, sh, H, W, band, ffts, flags=flags, slot=0)
            recs = ctx.download(stats, (n, len(FIELDS)), np.int64)
            frecs = ctx.download(ffts, (n,), FFT_DTYPE) if on_device else None
            planes = [ctx.download(b, (2, sh, sw), np.float32) for b in smalls] if want_small and not on_device else [None] * n
    out = []
    for k in range(n):
        st = {f: int(v) for f, v in zip(FIELDS, recs[k])}
        small = (planes[k][0], planes[k][1]) if want_small and not on_device else None
        fft_rec = {f: frecs[k][f].item() for f in FFT_DTYPE.names} if on_device else None
        out.append(finish(st, H, W, band, metric, augment_motion, ignore_highlights, mask_mode, small, fft_rec=fft_rec,
                          unit=UNIT16 if depth == 16 else 1))
    return out


def score_arrays(ctx, frames, metric, crop_ratio, augment_motion, ignore_highlights, mask_mode="none", red_index=0, fft=None):
    """9-tuples for a sequence of frames: uint8 ndarrays (H x W or H x W x C, RGB(A) order unless red_index = 2; uint16 ones too
    with GS360_FS_DEPTH16=device) or DeviceFrames already in device memory (decoded video frames, gs360/video.py).  Consecutive
    frames of one size and sample type, and for DeviceFrames one row stride, share a launch of up to GS360_MAX_FRAMES frames.  ctx None = the process's default context.  fft: where the fft / hybrid metrics' FFT runs, "host" or
    "device" (None = DEFAULT_FFT); with "device" no plane leaves the GPU."""
    fft = fft_mode(fft)
    frames = list(frames)
    shapes = [frame_shape(fr) for fr in frames]          # 16-bit / float sources and bad crops fail before any GPU work
    for shape in set(shapes):
        band_rows(shape[0], crop_ratio)
    ctx = ctx or default_context()
    out = []
    for i, j in _batches(frames, shapes):
        out += _score_batch(ctx, frames[i:j], shapes[i], metric, crop_ratio, augment_motion, ignore_highlights, mask_mode, red_index,
                            fft)
    return out


def _edge_batch(ctx, frames, shape, crop_ratio, red_index):
    H, W, Cn = shape
    n = len(frames)
    with device_frames(ctx, frames) as (bufs, stride, alloc):
        recs = alloc(n * capi.C.sizeof(capi.FrameEdge))
        with ctx.slot_locks[0]:
            ctx.frame_edge_dev(bufs, H, W, Cn, edge_band_rows(H, crop_ratio), recs, red_index=red_index, stride=stride, slot=0,
                               **depth_keyword(frame_depth(frames[0])))
            recs = ctx.download(recs, (n, len(EDGE_FIELDS)), np.int64)
    return [finish_edge({f: int(v) for f, v in zip(EDGE_FIELDS, r)}) for r in recs]


def edge_arrays(ctx, frames, crop_ratio, red_index=0):
    """9-tuples of the default ("ffmpeg") backend for a sequence of frames, batched and typed as score_arrays' (FS-EDGE v1; the
    backend ignores the metric, the highlights and the motion augmentation, FS:826-899)."""
    frames = list(frames)
    shapes = [frame_shape(fr) for fr in frames]
    ctx = ctx or default_context()
    out = []
    for i, j in _batches(frames, shapes):
        out += _edge_batch(ctx, frames[i:j], shapes[i], crop_ratio, red_index)
    return out


def decode(fp):
    """The image at fp as a uint8 ndarray, None when it cannot be read; a 16-bit image is a uint16 ndarray with
    GS360_FS_DEPTH16=device, else Gs360Error."""
    try:
        a = imageio.read_image(fp)
    except (imageio.ImageIOError, OSError):
        return None
    frame_shape(a)
    if a.dtype == np.uint16:
        with _ctx_lock:
            depth16_files.add(os.path.abspath(fp))
    return a


depth16_files = set()             # the 16-bit files decode has read (absolute paths); the CLI clears and counts them


def _source(decode_file, keep=False):
    """The pass's reader as a context: None under GS360_JPEG_DECODER=host (the default; the caller then decodes as ever), else
    gs360/framesource.py's Reader, which decodes baseline JPEG files on the device into gray DeviceFrames and hands every other file
    to decode_file.  keep: what it decodes may stay in an open framesource store."""
    if not jpegdec.device_decoder_enabled():
        return contextlib.nullcontext()
    from . import framesource             # (imports this module)
    return framesource.Reader(default_context(), decode_file, keep=keep)


def _host_frames(paths, ex, window):
    """(index, decode(path)) for every path, in order: decoding runs on the pool `ex`, at most `window` files ahead"""
    futs = collections.deque()
    nxt = 0
    while nxt < len(paths) or futs:
        while nxt < len(paths) and len(futs) < window:
            futs.append((nxt, ex.submit(decode, paths[nxt])))
            nxt += 1
        k, fut = futs.popleft()
        yield k, fut.result()


def _check_max_long(max_long):
    if max_long and max_long > 0:
        raise capi.Gs360Error(-4, "max_long > 0 is not implemented (the reference CLI runs with MAX_LONG = 0)")


def _edge_backend(backend, mask_mode):
    """Does a file take the edge pass: the "ffmpeg" backend, except under the circle mask; any other name is the OpenCV path, as in
    the reference (FS:480-483, FS:836-845)."""
    return backend == "ffmpeg" and mask_mode != "fisheye_circle"


def score_files(paths, metric, crop_ratio, max_long, augment_motion, ignore_highlights, mask_mode="none", workers=None, fft=None,
                backend="opencv", progress=None):
    """score_one_file (backend "opencv") or score_one_file_ffmpeg (backend "ffmpeg") over many paths: decoding on a thread pool
    overlaps the GPU batches; unreadable files give the reference's failure tuple.  Returns one tuple per path, in order.
    fft: as score_arrays.  progress(k), when given, is called as the number k of finished paths grows; what it raises ends the
    run."""
    fft = fft_mode(fft)
    edge = _edge_backend(backend, mask_mode)
    _check_max_long(max_long)
    if not edge:
        band_rows(1, crop_ratio)   # the reference's ValueError before any work
    paths = list(paths)
    ctx = default_context()
    out = [None] * len(paths)
    workers = workers or min(16, os.cpu_count() or 1)
    window = 2 * capi.MAX_FRAMES
    with concurrent.futures.ThreadPoolExecutor(max_workers=workers) as ex, _source(lambda fp: decode(fp), keep=True) as src:
        pending = []                      # (index, image) decoded, not yet scored
        done = [0]

        def finished(count):
            done[0] += count
            if progress:
                progress(done[0])

        def flush():
            if pending:
                imgs = [a for _, a in pending]
                res = edge_arrays(ctx, imgs, crop_ratio) if edge else \
                    score_arrays(ctx, imgs, metric, crop_ratio, augment_motion, ignore_highlights, mask_mode, fft=fft)
                if src:
                    src.release(imgs)
                for (k, _), r in zip(pending, res):
                    out[k] = r
                finished(len(pending))
                pending.clear()
        for k, a in (src.frames(paths, ex, window) if src else _host_frames(paths, ex, window)):
            if a is None:
                out[k] = FAILED
                finished(1)
                continue
            if pending and frame_shape(a) != frame_shape(pending[0][1]):
                flush()
            pending.append((k, a))
            if len(pending) == capi.MAX_FRAMES:
                flush()
        flush()
    return out


def score_one_file(fp, metric, crop_ratio, max_long, augment_motion, ignore_highlights, mask_mode="none", fft=None):
    """Drop-in for the reference's score_one_file (FS:902-1044) on the GPU.  fft: as score_arrays."""
    fft = fft_mode(fft)
    _check_max_long(max_long)
    with _source(lambda p: decode(p)) as src:
        a = src.read([fp])[0] if src else decode(fp)
        if a is None:
            return FAILED
        return score_arrays(None, [a], metric, crop_ratio, augment_motion, ignore_highlights, mask_mode, fft=fft)[0]


def score_one_file_ffmpeg(fp, metric, crop_ratio, max_long, augment_motion, ignore_highlights, mask_mode="none"):
    """Drop-in for the reference's score_one_file_ffmpeg (FS:826-899) on the GPU: the circle mask goes to score_one_file, as
    there; anything else is the edge pass, whatever the metric."""
    if mask_mode == "fisheye_circle":
        return score_one_file(fp, metric, crop_ratio, max_long, augment_motion, ignore_highlights, mask_mode=mask_mode)
    _check_max_long(max_long)
    with _source(lambda p: decode(p)) as src:
        a = src.read([fp])[0] if src else decode(fp)
        if a is None:
            return FAILED
        return edge_arrays(None, [a], crop_ratio)[0]


def record_mask_mode(record):
    """The mask of a record's frames: the circle for an X / Y fisheye pair record (FS:458-517, FS:1340-1361), else none."""
    return "fisheye_circle" if str(record.get("input_mode", "")).strip().lower() == "pair" else "none"


def score_one_record(record, metric, crop_ratio, max_long, augment_motion, ignore_highlights, score_backend="opencv", fft=None):
    """Drop-in for the reference's score_one_record (FS:458-517): a single image, or an X / Y fisheye pair scored with the circle
    mask and averaged field by field.  score_backend "ffmpeg" scores a single image with the edge pass (pairs always take the
    OpenCV path, as there).  fft: as score_arrays."""
    fft = fft_mode(fft)
    mask_mode = record_mask_mode(record)
    paths = list(record.get("file_paths", []))
    results = score_files(paths, metric, crop_ratio, max_long, augment_motion, ignore_highlights, mask_mode, workers=len(paths), fft=fft,
                          backend=score_backend)
    return average_tuples(results)


def average_tuples(results):
    """One record's 9-tuple from its files' (FS:502-517): every field the mean of its finite values, else the field's default."""
    if not results:
        return FAILED
    return tuple(mean_finite([r[k] for r in results], default=d) for k, d in enumerate(FAILED))


def score_records(records, metric, crop_ratio, max_long, augment_motion, ignore_highlights, score_backend="opencv", workers=None,
                  fft=None, progress=None):
    """score_one_record over a run's records, batched: the records of one mask mode go through one score_files call (so that
    decoding overlaps GS360_MAX_FRAMES-frame launches) and are averaged per record.  Returns one 9-tuple per record, in order.
    progress(k), when given, is called as the number k of finished records grows; what it raises ends the run."""
    out = [FAILED] * len(records)
    by_mode = {}
    for k, rec in enumerate(records):
        by_mode.setdefault(record_mask_mode(rec), []).append(k)
    base = 0
    for mask_mode, members in by_mode.items():
        paths, owner = [], []
        for k in members:
            for fp in records[k].get("file_paths", []):
                paths.append(fp)
                owner.append(k)

        def tick(count, base=base, n_paths=len(paths), n_recs=len(members)):
            progress(base + count * n_recs // max(1, n_paths))
        res = score_files(paths, metric, crop_ratio, max_long, augment_motion, ignore_highlights, mask_mode, workers=workers, fft=fft,
                          backend=score_backend, progress=tick if progress else None)
        per = {k: [] for k in members}
        for k, r in zip(owner, res):
            per[k].append(r)
        for k in members:
            out[k] = average_tuples(per[k])
        base += len(members)
    if progress:
        progress(len(records))
    return out
