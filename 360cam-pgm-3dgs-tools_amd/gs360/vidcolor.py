"""Decoded video frames to RGB on the GPU: the host half of a VID-COLOR v1 plan and its Python face.

Replaces the colour work of the reference's decoder filter `colorspace=iall=bt709:all=smpte170m[:trc=iec61966-2-1]`
(cli_tools/gs360_Video2Frames.py:464-466, gs360_360PerspCut.py:299-314): BT.709 Y'CbCr planes of 8 or 10 bits -> R'G'B' -> linear
light -> SMPTE-C primaries -> sRGB (or the Rec.709 curve with keep_rec709) -> interleaved RGB.  The integer first step runs in the
kernel from coefficients the library derives; the three tables of the float steps are built here in float64:

  primaries_matrix()   inv(M170) . M709 from the chromaticities of both standards
  linear_table()       R'G'B' level i / 16383 -> linear light, the Rec.709 constants gs360/color.py uses (DF:568-574)
  encode_table()       linear light -> output level, as 1024 cells of sqrt(l): (level at the cell's lower edge, rise over the cell)

No CPU path: converting needs a gs360 Context.
"""
import threading

import numpy as np

from . import capi

LEVELS = 1 << 14           # kVcLevels of csrc/gs360_vidsteps.h
ENC_CELLS = 1024           # kVcEnc
SUBSAMPLING = {"444": capi.VIDEO_444, "422": capi.VIDEO_422, "420": capi.VIDEO_420}
BT709 = ((0.640, 0.330), (0.300, 0.600), (0.150, 0.060), (0.3127, 0.3290))      # R, G, B, white (x, y)
SMPTE_C = ((0.630, 0.340), (0.310, 0.595), (0.155, 0.070), (0.3127, 0.3290))


def _rgb_to_xyz(chroma) -> np.ndarray:
    """RGB -> XYZ of a set of primaries and a white point: columns are the primaries' XYZ scaled so that white is (1, 1, 1)"""
    xyz = np.array([[x / y, 1.0, (1.0 - x - y) / y] for x, y in chroma], np.float64)
    prim, white = xyz[:3].T, xyz[3]
    return prim * np.linalg.solve(prim, white)[None, :]


def primaries_matrix() -> np.ndarray:
    """float64 3 x 3: linear BT.709 RGB -> linear SMPTE-C RGB (both D65)"""
    return np.linalg.solve(_rgb_to_xyz(SMPTE_C), _rgb_to_xyz(BT709))


def linear_table() -> np.ndarray:
    """float32 [16384]: the Rec.709 linearisation of v = i / 16383"""
    v = np.arange(LEVELS, dtype=np.float64) / (LEVELS - 1)
    lin = np.where(v < 0.081, v / 4.5, np.power((v + 0.099) / 1.099, 1.0 / 0.45))
    return np.clip(lin, 0.0, 1.0).astype(np.float32)


def encode_curve(lin: np.ndarray, keep_rec709: bool) -> np.ndarray:
    """float64 linear light in [0,1] -> the encoded value: sRGB, or the Rec.709 curve"""
    lin = np.asarray(lin, np.float64)
    if keep_rec709:
        return np.where(lin < 0.018, 4.5 * lin, 1.099 * np.power(lin, 0.45) - 0.099)
    return np.where(lin <= 0.0031308, 12.92 * lin, 1.055 * np.power(lin, 1.0 / 2.4) - 0.055)


def encode_table(keep_rec709: bool, outmax: int) -> np.ndarray:
    """float32 [1024][2]: cell i covers sqrt(l) * 1024 in [i, i + 1]; (a, b) = the output level at its lower edge and the float32
    difference to the level at its upper edge, so that the kernel's a + b * f runs from one edge to the other"""
    t = np.arange(ENC_CELLS + 1, dtype=np.float64) / ENC_CELLS
    edge = (np.clip(encode_curve(t * t, keep_rec709), 0.0, 1.0) * outmax).astype(np.float32)
    return np.ascontiguousarray(np.stack([edge[:-1], edge[1:] - edge[:-1]], axis=1), np.float32)


class VideoColor:
    """The tables of one (depth, range, curve, output depth) and, per Context, its plan.  out_bits None is the depth's own pairing
    (uint8 from 8-bit planes, uint16 from 10-bit ones); 8 with depth 10 is VID-FEED v1's uint8 RGB from 10-bit planes."""

    def __init__(self, depth: int, full_range: bool = False, keep_rec709: bool = False, out_bits=None):
        if depth not in (8, 10):
            raise ValueError("VID-COLOR v1 takes 8- and 10-bit planes (got {})".format(depth))
        if out_bits is None:
            out_bits = 8 if depth == 8 else 16
        if (int(depth), int(out_bits)) not in ((8, 8), (10, 16), (10, 8)):
            raise ValueError("no {}-bit RGB from {}-bit planes: 8 from 8, 16 from 10 and 8 from 10 are converted".format(out_bits, depth))
        self.depth, self.full_range, self.keep_rec709 = int(depth), bool(full_range), bool(keep_rec709)
        self.out_bits = int(out_bits)
        self.in_dtype = np.dtype(np.uint8 if depth == 8 else np.uint16)
        self.out_dtype = np.dtype(np.uint8 if self.out_bits == 8 else np.uint16)
        self.outmax = 255 if self.out_bits == 8 else 65535
        self.matrix = primaries_matrix().astype(np.float32)
        self.linear = linear_table()
        self.encode = encode_table(self.keep_rec709, self.outmax)
        self._plans = {}
        self._lock = threading.Lock()

    def plan(self, ctx):
        with self._lock:
            p = self._plans.get(ctx)
            if p is None:
                p = self._plans[ctx] = ctx.video_plan(self.depth, self.full_range, self.keep_rec709, self.matrix, self.linear, self.encode,
                                                           out_bits=self.out_bits)
            return p

    def convert_dev(self, ctx, jobs, slot: int = 0) -> None:
        """jobs: sequence of (y, cb, cr, W, H, subsampling, dst[, y_stride, cb_stride, cr_stride, dst_stride]) with DeviceBuffers or
        device addresses, subsampling one of "420" / "422" / "444"; at most capi.MAX_FRAMES per call.  Asynchronous on `slot`."""
        ctx.video_rgb_dev(self.plan(ctx), [(j[0], j[1], j[2], j[3], j[4], SUBSAMPLING[j[5]]) + tuple(j[6:]) for j in jobs], slot=slot)

    def convert(self, ctx, y, u, v, slot: int = 0) -> np.ndarray:
        """Host convenience: upload three planes (the subsampling follows from their shapes), convert, download H x W x 3."""
        y, u, v = (np.ascontiguousarray(p, self.in_dtype) for p in (y, u, v))
        H, W = y.shape
        sub = {(H, W): "444", (H, (W + 1) // 2): "422", ((H + 1) // 2, (W + 1) // 2): "420"}.get(u.shape)
        if sub is None or v.shape != u.shape:
            raise ValueError("chroma planes {} / {} fit no subsampling of a {} x {} frame".format(u.shape, v.shape, W, H))
        with ctx.slot_locks[slot]:
            bufs = [ctx.to_device(p, slot=slot) for p in (y, u, v)]
            dst = ctx.alloc(H * W * 3 * self.out_dtype.itemsize)
            try:
                self.convert_dev(ctx, [(bufs[0], bufs[1], bufs[2], W, H, sub, dst)], slot=slot)
                return ctx.download(dst, (H, W, 3), dtype=self.out_dtype, slot=slot)
            finally:
                for b in bufs + [dst]:
                    ctx.free(b)

    def close(self) -> None:
        with self._lock:
            for ctx, p in self._plans.items():
                if ctx.handle:
                    ctx.video_plan_free(p)
            self._plans.clear()
