"""Finishing segmentation masks on the device (MSK-SPEC v1).

What gs360_SegmentationMaskTool.py runs on every image after the network (SEG:680-781): close with a small ellipse, dilate with a
larger one, fuse to the frame edges, OR in the manual add layer, count, and write the mask or compose it with the image.  The raw masks
come from any segmenter (or none: manual layers alone); the network itself is not part of this package.  One gs360_mask_finish_u8 call
(csrc/gs360_maskmorph.hip) finishes a batch; the elements reach the kernels as data, built here by structuring_rows.
"""
import math
import pathlib
from dataclasses import dataclass

import numpy as np

from . import capi

KINDS = {"mask": capi.MASK_OUT_MASK, "rgba": capi.MASK_OUT_RGBA, "keep": capi.MASK_OUT_KEEP, "remove": capi.MASK_OUT_REMOVE}
_CHANNELS = {"mask": 1, "rgba": 4, "keep": 3, "remove": 3}
MAX_EXPAND = (capi.MASK_MAX_ELEMENT - 1) // 2          # the largest p: an element of 1025 x 1025


def structuring_rows(kw, kh):
    """-> ([(j1, j2)] per element row: the half-open span of set columns, (ax, ay) = (kw // 2, kh // 2)) of the kw x kh ellipse as
    OpenCV 4.x's getStructuringElement(MORPH_ELLIPSE, (kw, kh)) builds it: r = kh // 2, c = kw // 2, per row dy = i - r and
    dx = rint(c * sqrt((r^2 - dy^2) / r^2)) in double, half to even; columns [max(c - dx, 0), min(c + dx + 1, kw)).  With r = 0 the
    square root's argument is 0 (1 / r^2 is taken as 0): a (2s+1) x 1 element is its centre alone; with c = 0 every row is [0, 1):
    a 1 x (2s+1) element is a full column."""
    kw, kh = int(kw), int(kh)
    if kw < 1 or kh < 1:
        raise ValueError(f"element of {kw} x {kh}")
    r, c = kh // 2, kw // 2
    inv_r2 = 1.0 / (float(r) * r) if r else 0.0
    rows = []
    for i in range(kh):
        dy = i - r
        dx = int(round(c * math.sqrt((r * r - dy * dy) * inv_r2)))      # round(): half to even, as cvRound
        rows.append((max(c - dx, 0), min(c + dx + 1, kw)))
    return rows, (c, r)


def _rint(v):
    """to the nearest integer, a tie to the even one (Python's round, which the reference's amounts go through)"""
    return int(round(v))


def resolve_expand_pixels(mode="pixels", pixels=15, percent=1.0, image_shape=None):
    """the expansion p in pixels (the rule of SEG:359-381): in "pixels" mode `pixels`, in "percent" mode `percent` hundredths of the
    longer side of image_shape = (H, W) (0 without a shape); either one to the nearest integer, a tie to the even one, and never
    below 0.  An empty mode means "pixels"; any other word is a ValueError."""
    key = ("" if mode is None else str(mode)).strip().lower() or "pixels"
    if key not in ("pixels", "percent"):
        raise ValueError(f"mask expand mode must be 'pixels' or 'percent' (got {mode!r})")
    if key == "pixels":
        amount = float(pixels)
    elif image_shape is None or len(image_shape) < 2:
        amount = 0.0
    else:
        amount = max(int(image_shape[0]), int(image_shape[1])) * (float(percent) / 100.0)
    return max(0, _rint(amount))


def fuse_spread(edge_fuse_pixels):
    """-> (f, s): the strips' width and the side seeds' spread, s = 0.35 f to the nearest integer and at least 1 (SEG:444-452)"""
    f = max(0, int(edge_fuse_pixels))
    return f, max(1, _rint(f * 0.35))


def _is_camera(token):
    """a view id's first part: one letter, or a number of two or more digits"""
    return (len(token) == 1 and "A" <= token <= "Z") or (len(token) >= 2 and token.isdecimal())


def _is_tilt(token):
    """a view id's optional second part: U or D, alone or followed by digits"""
    return token[:1] in ("U", "D") and (len(token) == 1 or token[1:].isdecimal())


def view_id(stem):
    """-> the view id a file stem ends in, read in upper case after an underscore (A, A_U, 12_D20), or None (the grammar of
    SEG:566-572): the longest id wins, so `x_A_D` is camera A tilted down and `x_7_D` is camera D"""
    parts = stem.upper().split("_")
    if len(parts) >= 3 and _is_tilt(parts[-1]) and _is_camera(parts[-2]):
        return f"{parts[-2]}_{parts[-1]}"
    if len(parts) >= 2 and _is_camera(parts[-1]):
        return parts[-1]
    return None


def manual_key(path):
    """the manual layer's key of an image path (SEG:575-580): `view__<ID>` for a stem that ends in a view id, else `file__<stem>`;
    the add layer is `<key>__add.png`"""
    stem = pathlib.PurePath(path).stem
    vid = view_id(stem)
    return f"view__{vid}" if vid else f"file__{stem}"


@dataclass
class Params:
    close: int = 5
    expand_mode: str = "pixels"
    expand_pixels: int = 15
    expand_percent: float = 1.0
    edge_fuse_pixels: int = 25
    thresh: int = 0


def _rows_array(kw, kh, cache):
    if (kw, kh) not in cache:
        cache[(kw, kh)] = np.ascontiguousarray(structuring_rows(kw, kh)[0], dtype=np.int32)
    return cache[(kw, kh)]


def build_jobs(shapes, params, kind="mask", invert=True):
    """shapes: [(H, W)] -> ([capi.MaskJob] with everything but the pointers and strides filled, the host arrays they point into).
    Raises ValueError for an unknown kind and for edge_fuse_pixels > min(H, W) (the reference's slices turn negative there)."""
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {sorted(KINDS)} (got {kind!r})")
    close = max(1, int(params.close))
    f, s = fuse_spread(params.edge_fuse_pixels)
    cache, jobs = {}, []
    for H, W in shapes:
        H, W = int(H), int(W)
        if f > min(H, W):
            raise ValueError(f"edge_fuse_pixels {f} exceeds the {W} x {H} mask's shorter side")
        p = resolve_expand_pixels(params.expand_mode, params.expand_pixels, params.expand_percent, (H, W))
        j = capi.MaskJob()
        j.H, j.W, j.thresh = H, W, int(params.thresh)
        j.fuse, j.spread, j.kind, j.invert = f, s, KINDS[kind], 1 if invert else 0
        if close > 1:
            j.close_kw = j.close_kh = close
            if close <= capi.MASK_MAX_ELEMENT:
                j.close_rows = _rows_array(close, close, cache).ctypes.data
        if p > 0:
            j.expand_kw = j.expand_kh = 2 * p + 1
            if p <= MAX_EXPAND:                          # (beyond: the call answers GS360_ERR_UNSUPPORTED before it reads the rows)
                j.expand_rows = _rows_array(2 * p + 1, 2 * p + 1, cache).ctypes.data
        jobs.append(j)
    return jobs, cache


def finish_device(ctx, masks, params=None, adds=None, images=None, kind="mask", invert=True, slot=0):
    """(the caller holds `slot`) masks: per image an H x W uint8 ndarray or an (H, W) tuple (no detection: all clear) ->
    ([(DeviceBuffer, H, W, C, 1, 0)] outputs left on the device, in pngenc's item form, counts as a uint32 array).  adds: None or
    per image None / an H x W uint8 layer (set where > 0); images: per image an H x W x 3 uint8 array, needed by every kind but
    "mask".  The output buffers are the caller's to free."""
    params = params or Params()
    n = len(masks)
    adds = list(adds) if adds is not None else [None] * n
    images = list(images) if images is not None else [None] * n
    if len(adds) != n or len(images) != n:
        raise ValueError("one add layer and one image per mask (or None)")
    shapes = [tuple(m) if isinstance(m, tuple) else np.asarray(m).shape[:2] for m in masks]
    jobs, keep = build_jobs(shapes, params, kind, invert)
    if not n:
        return [], np.zeros(0, np.uint32)
    owned, outs = [], []

    def plane(a, shape, what):
        a = np.ascontiguousarray(a, dtype=np.uint8)
        if a.shape != shape:
            raise ValueError(f"{what} of shape {a.shape}, expected {shape}")
        owned.append(ctx.to_device(a, slot))
        return owned[-1].ptr
    try:
        C = _CHANNELS[kind]
        for j, m, a, im, (H, W) in zip(jobs, masks, adds, images, shapes):
            if not isinstance(m, tuple):
                j.src = plane(m, (H, W), "mask")
            if a is not None:
                j.add = plane(a, (H, W), "add layer")
            if kind != "mask":
                if im is None:
                    raise ValueError(f"kind {kind!r} needs the images")
                j.image = plane(im, (H, W, 3), "image")
            outs.append(ctx.alloc(H * W * C))
            j.dst = outs[-1].ptr
        scratch = ctx.alloc(max(ctx.mask_finish_scratch(jobs), 256))
        owned.append(scratch)
        d_counts = ctx.alloc(4 * n)
        owned.append(d_counts)
        ctx.mask_finish_dev(jobs, scratch, d_counts, slot)
        counts = ctx.download(d_counts, (n,), np.uint32, slot)       # (synchronises the slot: the staged inputs may go)
        del keep
        return [(o, H, W, C, 1, 0) for o, (H, W) in zip(outs, shapes)], counts
    except BaseException:
        for o in outs:
            ctx.free(o)
        raise
    finally:
        for b in owned:
            ctx.free(b)


def finish(ctx, masks, params=None, adds=None, images=None, kind="mask", invert=True, slot=0):
    """finish_device with the outputs brought back: -> ([H x W (kind "mask") or H x W x C uint8 arrays], counts)"""
    with ctx.slot_locks[slot]:
        items, counts = finish_device(ctx, masks, params, adds, images, kind, invert, slot)
        try:
            return [ctx.download(o, (H, W) if C == 1 else (H, W, C), np.uint8, slot) for o, H, W, C, _b, _s in items], counts
        finally:
            for it in items:
                ctx.free(it[0])
