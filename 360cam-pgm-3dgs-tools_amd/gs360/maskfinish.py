"""Finishing segmentation masks on the device (MSK-SPEC v1).

What gs360_SegmentationMaskTool.py runs on every image after the network (SEG:680-781): close with a small ellipse, dilate with a
larger one, fuse to the frame edges, OR in the manual add layer, count, and write the mask or compose it with the image.  The raw masks
come from any segmenter (or none: manual layers alone); the network itself is not part of this package.  One gs360_mask_finish_u8 call
(csrc/gs360_maskmorph.hip) finishes a batch; the elements reach the kernels as data, built here by structuring_rows.

With the shadow estimate (MSK-SHADOW v1, SEG:499-558 between the close and the expansion) two more calls come first
(csrc/gs360_maskshadow.hip): gs360_mask_shadow_candidates_u8 leaves the person plane, its count and the shadow candidates on the device,
the host turns the count into element sizes (shadow_sizes), and gs360_mask_shadow_merge_u8 writes M = person | shadow, which the
finishing call then reads from device memory.  The Gaussian's weights and the saturation divisors are data as well.

Inpainting (MSK-INPAINT v1, the reference's --mode inpaint, SEG:809-815) comes after the chain: the finished mask, written with kind
"mask" and invert off, is the fill mask F of gs360_mask_inpaint_u8 (csrc/gs360_maskinpaint.hip), which fills the image in place.
"""
import dataclasses
import math
import os
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


@dataclass
class ShadowParams:
    """estimate_shadow_mask's parameters and their defaults (SEG:63-71)"""
    t: float = 0.82
    sigma: float = 21
    near_px: int = 25
    min_area: int = 160
    delta_min: float = 12
    sat_max: int = 115


SHADOW_MAX_NEAR, SHADOW_NEAR_SCALE, SHADOW_CLOSE_SCALE = 128, 0.2, 0.2      # SEG:69-71


def shadow_mode_from_env():
    """-> True when --include_shadow runs the device estimate.  GS360_MASK_SHADOW = off (default: the flag is refused as before;
    the estimate's parity with cv2 is not pinned) | device."""
    mode = os.environ.get("GS360_MASK_SHADOW", "off")
    if mode not in ("off", "device"):
        raise ValueError(f"GS360_MASK_SHADOW must be off or device (got {mode!r})")
    return mode == "device"


INPAINT_RADIUS = 5                                       # cv2.inpaint's inpaintRadius in the reference (SEG:73)


def inpaint_mode_from_env():
    """-> True when --mode inpaint runs the device stage.  GS360_MASK_INPAINT = off (default: the mode is refused as before; the
    stage's parity with cv2.inpaint is not pinned) | device."""
    mode = os.environ.get("GS360_MASK_INPAINT", "off")
    if mode not in ("off", "device"):
        raise ValueError(f"GS360_MASK_INPAINT must be off or device (got {mode!r})")
    return mode == "device"


def inpaint_offsets(radius=INPAINT_RADIUS):
    """-> (n x 2 int32 (dy, dx), |r| and 1 / |r|^2 as float32): MSK-INPAINT's neighbourhood, the offsets with
    0 < dy^2 + dx^2 <= radius^2 in row-major order; both numbers are taken in double and rounded to float32, as the library does"""
    radius = int(radius)
    if not capi.INPAINT_MIN_RADIUS <= radius <= capi.INPAINT_MAX_RADIUS:
        raise ValueError(f"inpaint radius must be {capi.INPAINT_MIN_RADIUS}..{capi.INPAINT_MAX_RADIUS} (got {radius})")
    dy, dx = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    d = (dy * dy + dx * dx).reshape(-1)
    use = (d > 0) & (d <= radius * radius)
    pairs = np.stack([dy.reshape(-1)[use], dx.reshape(-1)[use]], axis=1).astype(np.int32)
    d = d[use].astype(np.float64)
    return pairs, np.sqrt(d).astype(np.float32), (1.0 / d).astype(np.float32)


def gaussian_weights(sigma):
    """-> the float32 kernel cv2.GaussianBlur(float image, (0, 0), sigma) filters with along either axis, all ksize of it:
    ksize = rint(8 sigma + 1) | 1 (OpenCV's rule for a source that is not 8-bit), exp(-x^2 / (2 sigma^2)) in double, divided by the
    double sum, rounded to float32.  The kernels take the half from the centre outward."""
    sigma = float(sigma)
    if not sigma > 0:
        raise ValueError(f"sigma must be positive (got {sigma})")
    ksize = _rint(sigma * 8 + 1) | 1
    x = np.arange(ksize, dtype=np.float64) - (ksize - 1) * 0.5
    k = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return (k / k.sum()).astype(np.float32)


def sat_div_table():
    """-> the 256 int32 divisors of cv2's 8-bit RGB2HSV saturation, S = (d sdiv[v] + 2048) >> 12: sdiv[0] = 0,
    sdiv[i] = rint(1044480 / i) in double, a tie to the even one"""
    t = np.zeros(256, np.int32)
    t[1:] = np.rint(1044480.0 / np.arange(1, 256, dtype=np.float64)).astype(np.int32)
    return t


def shadow_sizes(count, near_px=25):
    """person pixels -> (k, close_k): the sides of the near-region ellipse and of the closing ellipse, in the reference's own
    expressions (SEG:527-540)"""
    n = max(1, int(count))
    near = int(max(int(near_px), min(SHADOW_MAX_NEAR, math.sqrt(n) * SHADOW_NEAR_SCALE)))
    k = max(3, near | 1)
    return k, max(5, int(round(k * SHADOW_CLOSE_SCALE)) | 1)


def _rows_array(kw, kh, cache):
    if (kw, kh) not in cache:
        cache[(kw, kh)] = np.ascontiguousarray(structuring_rows(kw, kh)[0], dtype=np.int32)
    return cache[(kw, kh)]


def set_element(j, name, k, cache):
    """the k x k ellipse as element `name` (close, expand, near, sclose, open) of job j; cache keeps the rows alive"""
    setattr(j, name + "_kw", k)
    setattr(j, name + "_kh", k)
    if k <= capi.MASK_MAX_ELEMENT:                       # (beyond: the call answers GS360_ERR_UNSUPPORTED before it reads the rows)
        setattr(j, name + "_rows", _rows_array(k, k, cache).ctypes.data)


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
            set_element(j, "close", close, cache)
        if p > 0:
            set_element(j, "expand", 2 * p + 1, cache)
        jobs.append(j)
    return jobs, cache


def _device_plane(ctx, a, shape, what, owned, slot):
    """-> the device address of a uint8 array of `shape`: a DeviceBuffer's own, else that of a fresh upload, which joins `owned`"""
    if isinstance(a, capi.DeviceBuffer):
        return a.ptr
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.shape != shape:
        raise ValueError(f"{what} of shape {a.shape}, expected {shape}")
    owned.append(ctx.to_device(a, slot))
    return owned[-1].ptr


def _shapes(masks):
    """[(H, W)] of masks given as arrays, (H, W) or (H, W, DeviceBuffer)"""
    return [tuple(m[:2]) if isinstance(m, tuple) else np.asarray(m).shape[:2] for m in masks]


def _source_plane(ctx, j, m, shape, owned, slot):
    """job j's raw mask: an array is uploaded, a DeviceBuffer is taken as it is, a bare shape leaves it NULL (all clear)"""
    if not isinstance(m, tuple):
        j.src = _device_plane(ctx, m, shape, "mask", owned, slot)
    elif len(m) == 3:
        j.src = m[2].ptr


def _download_and_free(ctx, items, slot):
    """finish_device's items brought back as H x W (one channel) or H x W x C arrays; their buffers are freed"""
    try:
        return [ctx.download(o, (H, W) if C == 1 else (H, W, C), np.uint8, slot) for o, H, W, C, _b, _s in items]
    finally:
        for it in items:
            ctx.free(it[0])


def finish_device(ctx, masks, params=None, adds=None, images=None, kind="mask", invert=True, slot=0):
    """(the caller holds `slot`) masks: per image an H x W uint8 ndarray, an (H, W) tuple (no detection: all clear) or an
    (H, W, DeviceBuffer) tuple (a mask that is on the device already) ->
    ([(DeviceBuffer, H, W, C, 1, 0)] outputs left on the device, in pngenc's item form, counts as a uint32 array).  adds: None or
    per image None / an H x W uint8 layer (set where > 0); images: per image an H x W x 3 uint8 array or a DeviceBuffer holding
    one, needed by every kind but "mask".  The output buffers are the caller's to free; buffers that came in stay the caller's."""
    params = params or Params()
    n = len(masks)
    adds = list(adds) if adds is not None else [None] * n
    images = list(images) if images is not None else [None] * n
    if len(adds) != n or len(images) != n:
        raise ValueError("one add layer and one image per mask (or None)")
    shapes = _shapes(masks)
    jobs, keep = build_jobs(shapes, params, kind, invert)
    if not n:
        return [], np.zeros(0, np.uint32)
    owned, outs = [], []
    try:
        C = _CHANNELS[kind]
        for j, m, a, im, (H, W) in zip(jobs, masks, adds, images, shapes):
            _source_plane(ctx, j, m, (H, W), owned, slot)
            if a is not None:
                j.add = _device_plane(ctx, a, (H, W), "add layer", owned, slot)
            if kind != "mask":
                if im is None:
                    raise ValueError(f"kind {kind!r} needs the images")
                j.image = _device_plane(ctx, im, (H, W, 3), "image", owned, slot)
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
        return _download_and_free(ctx, items, slot), counts


def shadow_device(ctx, masks, images, params=None, shadow=None, slot=0):
    """(the caller holds `slot`) the person masks of finish_device (ndarrays or (H, W) tuples) and their H x W x 3 uint8 images
    (ndarrays or DeviceBuffers) -> ([DeviceBuffer of H x W bytes, 0 / 255] M = closed person mask | shadow estimate, counts of M as a
    uint32 array).  params: the finishing Params (close and thresh are used here); shadow: ShadowParams.  The buffers are the
    caller's to free."""
    params, shadow = params or Params(), shadow or ShadowParams()
    n = len(masks)
    if len(images) != n:
        raise ValueError("one image per mask")
    if not n:
        return [], np.zeros(0, np.uint32)
    shapes = _shapes(masks)
    weights, sdiv, cache = gaussian_weights(shadow.sigma), sat_div_table(), {}
    half = np.ascontiguousarray(weights[len(weights) // 2:])
    close = max(1, int(params.close))
    owned, outs, jobs = [], [], []

    try:
        for m, im, (H, W) in zip(masks, images, shapes):
            j = capi.ShadowJob()
            j.H, j.W, j.thresh = int(H), int(W), int(params.thresh)
            j.radius, j.weights, j.sdiv = len(half) - 1, half.ctypes.data, sdiv.ctypes.data
            j.t, j.delta_min, j.sat_max = float(shadow.t), float(shadow.delta_min), int(shadow.sat_max)
            j.min_area = max(1, min(int(shadow.min_area), 2 ** 31 - 1))
            if close > 1:
                set_element(j, "close", close, cache)
            _source_plane(ctx, j, m, (H, W), owned, slot)
            j.image = _device_plane(ctx, im, (H, W, 3), "image", owned, slot)
            outs.append(ctx.alloc(H * W))
            j.dst = outs[-1].ptr
            jobs.append(j)
        scratch = ctx.alloc(ctx.mask_shadow_scratch(jobs))
        owned.append(scratch)
        d_counts = ctx.alloc(4 * n)
        owned.append(d_counts)
        ctx.mask_shadow_candidates_dev(jobs, scratch, d_counts, slot)
        person = ctx.download(d_counts, (n,), np.uint32, slot)
        for j, count in zip(jobs, person):               # the count -> size rule stays on the host
            k, close_k = shadow_sizes(int(count), shadow.near_px)
            set_element(j, "near", k, cache)
            set_element(j, "sclose", close_k, cache)
            set_element(j, "open", 3, cache)
        ctx.mask_shadow_merge_dev(jobs, scratch, d_counts, slot)
        counts = ctx.download(d_counts, (n,), np.uint32, slot)
        del cache
        return outs, counts
    except BaseException:
        for o in outs:
            ctx.free(o)
        raise
    finally:
        for b in owned:
            ctx.free(b)


def finish_with_shadow_device(ctx, masks, params=None, shadow=None, adds=None, images=None, kind="mask", invert=True, slot=0):
    """finish_device with the shadow estimate between the close and the expansion (the reference's --include_shadow): the images are
    needed by every kind.  M stays on the device between the two stages, and so do the images."""
    params = params or Params()
    if images is None:
        raise ValueError("the shadow estimate needs the images")
    n = len(masks)
    shapes = _shapes(masks)
    d_images, merged = [], []
    try:
        for im, (H, W) in zip(images, shapes):
            _device_plane(ctx, im, (H, W, 3), "image", d_images, slot)
        if len(d_images) != n:
            raise ValueError("one image per mask")
        merged, _counts = shadow_device(ctx, masks, d_images, params, shadow, slot)
        rest = dataclasses.replace(params, close=1, thresh=0)        # M is closed and holds 0 / 255
        return finish_device(ctx, [(H, W, m) for (H, W), m in zip(shapes, merged)], rest, adds, d_images if kind != "mask" else None,
                             kind, invert, slot)
    finally:
        for b in d_images + merged:
            ctx.free(b)


def finish_with_shadow(ctx, masks, params=None, shadow=None, adds=None, images=None, kind="mask", invert=True, slot=0):
    """finish_with_shadow_device with the outputs brought back: -> ([H x W (kind "mask") or H x W x C uint8 arrays], counts)"""
    with ctx.slot_locks[slot]:
        items, counts = finish_with_shadow_device(ctx, masks, params, shadow, adds, images, kind, invert, slot)
        return _download_and_free(ctx, items, slot), counts


def inpaint_device(ctx, images, fills, radius=INPAINT_RADIUS, slot=0):
    """(the caller holds `slot`) images: [(DeviceBuffer of H x W x 3 bytes, H, W)], filled in place; fills: per image a DeviceBuffer
    of H x W bytes, set where > 0 (a finished mask of kind "mask" with invert off) -> K per image as a uint32 array: the levels
    that were filled, 0 for a mask that is empty or covers the image (the image is left alone then).  Returns when the kernels are
    done."""
    n = len(images)
    if len(fills) != n:
        raise ValueError("one fill mask per image")
    if not n:
        return np.zeros(0, np.uint32)
    jobs = []
    for (buf, H, W), fill in zip(images, fills):
        j = capi.InpaintJob()
        j.image, j.fill, j.H, j.W, j.radius = buf.ptr, fill.ptr, int(H), int(W), int(radius)
        jobs.append(j)
    owned = []
    try:
        owned.append(ctx.alloc(ctx.mask_inpaint_scratch(jobs)))
        owned.append(ctx.alloc(4 * n))
        ctx.mask_inpaint_dev(jobs, owned[0], owned[1], slot)
        return ctx.download(owned[1], (n,), np.uint32, slot)
    finally:
        for b in owned:
            ctx.free(b)


def finish_with_inpaint_device(ctx, masks, params=None, adds=None, images=None, shadow=None, radius=INPAINT_RADIUS, slot=0):
    """(the caller holds `slot`) the finishing chain with kind "mask" and invert off -- after the shadow estimate when `shadow` is a
    ShadowParams or True (the defaults) -- and the finished masks' regions of the images inpainted ->
    ([(DeviceBuffer, H, W, 3, 1, 0)] the filled images left on the device, in pngenc's item form, K per image).  images: per mask
    an H x W x 3 uint8 array; its copy on the device serves the shadow estimate, is filled in place and is the output.  The masks
    never leave the device.  The output buffers are the caller's to free."""
    params = params or Params()
    if images is None or len(images) != len(masks):
        raise ValueError("inpainting needs one image per mask")
    shapes = _shapes(masks)
    d_images, merged, finished = [], [], []
    try:
        for im, (H, W) in zip(images, shapes):
            if isinstance(im, capi.DeviceBuffer):
                raise ValueError("inpainting fills its own copy of an image: give arrays")
            _device_plane(ctx, im, (H, W, 3), "image", d_images, slot)
        if shadow:                                       # as finish_with_shadow_device, on the images that are resident already
            merged, _counts = shadow_device(ctx, masks, d_images, params, shadow if isinstance(shadow, ShadowParams) else None, slot)
            params = dataclasses.replace(params, close=1, thresh=0)
            masks = [(H, W, m) for (H, W), m in zip(shapes, merged)]
        finished, _counts = finish_device(ctx, masks, params, adds, None, "mask", False, slot)
        levels = inpaint_device(ctx, [(b, H, W) for b, (H, W) in zip(d_images, shapes)], [it[0] for it in finished], radius, slot)
        items, d_images = [(b, H, W, 3, 1, 0) for b, (H, W) in zip(d_images, shapes)], []
        return items, levels
    finally:
        for b in d_images + merged + [it[0] for it in finished]:
            ctx.free(b)


def finish_with_inpaint(ctx, masks, params=None, adds=None, images=None, shadow=None, radius=INPAINT_RADIUS, slot=0):
    """finish_with_inpaint_device with the outputs brought back: -> ([H x W x 3 uint8 arrays], K per image)"""
    with ctx.slot_locks[slot]:
        items, levels = finish_with_inpaint_device(ctx, masks, params, adds, images, shadow, radius, slot)
        return _download_and_free(ctx, items, slot), levels
