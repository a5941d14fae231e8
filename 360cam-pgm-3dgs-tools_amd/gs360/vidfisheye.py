"""Decoded fisheye frames to pinhole views in RGB on the GPU: the Python face of VID-FISHEYE v1.

Replaces the reference's --fisheye-perspective filter graph (cli_tools/gs360_Video2Frames.py:467-493),
`v360=<fisheye|equisolid>:rectilinear:ih_fov=F:iv_fov=F:h_fov=..:v_fov=..:interp=cubic` + colorspace + `scale=S:S`: each plane of a
decoded Y'CbCr frame is interpolated (v360's cubic) at the place of every view pixel in the ideal fisheye image and the three samples
go through VID-COLOR v1's conversion, in one kernel (gs360_video_fisheye_rgb).

  view_from_args()   the reference's geometry: fields of view from the focal length, clamped and rounded as its filter string is
  FisheyeStage       a VideoColor (depth, range, curve -> tables and plan) and the call
  mode_from_env()    GS360_V2F_FISHEYE: unset = the drop-in refuses the flag as before, `device` = this stage

No CPU path: converting needs a gs360 Context.
"""
import math
import os
from collections import namedtuple

import numpy as np

from . import capi
from .vidcolor import SUBSAMPLING, VideoColor

SENSOR_WIDTH_MM = 36.0                 # FISHEYE_SENSOR_WIDTH_MM (V2F:29)
PROJECTIONS = {"equidistant": capi.FISHEYE_EQUIDISTANT, "equisolid": capi.FISHEYE_EQUISOLID}
ENV = "GS360_V2F_FISHEYE"
MAX_SIDE = capi.FISHEYE_MAX_SIDE       # the largest source side and view size

FisheyeView = namedtuple("FisheyeView", "projection size input_fov_deg h_fov_deg v_fov_deg")


def _six(v: float) -> float:
    """a value as the reference's filter string carries it (`{v:.6f}`)"""
    return float(f"{v:.6f}")


def view_from_args(focal_mm: float, size: int, projection: str, input_fov: float) -> FisheyeView:
    """V2F:467-482: hfov from the focal length over a 36 mm sensor, vfov of the square view, the lens circle's fov; each clamped, then
    rounded to six decimals.  `projection` is `equidistant` or `equisolid`."""
    if projection not in PROJECTIONS:
        raise ValueError("projection must be equidistant or equisolid (got {!r})".format(projection))
    focal_mm = max(float(focal_mm), 1e-6)
    size = max(int(size), 1)
    ifov = max(1.0, min(360.0, float(input_fov)))
    hfov = math.degrees(2.0 * math.atan(SENSOR_WIDTH_MM / (2.0 * focal_mm)))
    hfov = max(1.0, min(179.0, hfov))
    vfov = math.degrees(2.0 * math.atan(math.tan(math.radians(hfov) / 2.0) * (size / float(size))))
    vfov = max(1.0, min(179.0, vfov))
    return FisheyeView(projection, size, _six(ifov), _six(hfov), _six(vfov))


def mode_from_env(environ=None) -> bool:
    """GS360_V2F_FISHEYE: unset or empty -> False, `device` -> True, anything else is an error"""
    value = (os.environ if environ is None else environ).get(ENV, "")
    if value == "":
        return False
    if value == "device":
        return True
    raise ValueError("{} must be `device` or unset (got {!r})".format(ENV, value))


class FisheyeStage:
    """A view and the colour tables of one (depth, range, curve)."""

    def __init__(self, view: FisheyeView, depth: int, full_range: bool = False, keep_rec709: bool = False, color: VideoColor = None):
        self.view = view
        self.color = color if color is not None else VideoColor(depth, full_range, keep_rec709)
        self._owns = color is None
        self.in_dtype = self.color.in_dtype

    def convert_dev(self, ctx, jobs, slot: int = 0) -> None:
        """jobs: sequence of (y, cb, cr, W, H, subsampling, dst[, y_stride, cb_stride, cr_stride, dst_stride]) as for
        VideoColor.convert_dev; every job has the same W x H and its dst holds size x size x 3 samples.  Asynchronous on `slot`."""
        if not jobs:
            return
        v = self.view
        ctx.video_fisheye_rgb_dev(self.color.plan(ctx), (PROJECTIONS[v.projection], v.size, jobs[0][3], jobs[0][4], v.input_fov_deg,
                                                         v.h_fov_deg, v.v_fov_deg),
                                  [(j[0], j[1], j[2], j[3], j[4], SUBSAMPLING[j[5]]) + tuple(j[6:]) for j in jobs], slot=slot)

    def convert(self, ctx, y, u, v, slot: int = 0) -> np.ndarray:
        """Host convenience: upload three planes (the subsampling follows from their shapes), render, download size x size x 3."""
        y, u, v = (np.ascontiguousarray(p, self.in_dtype) for p in (y, u, v))
        H, W = y.shape
        sub = {(H, W): "444", (H, (W + 1) // 2): "422", ((H + 1) // 2, (W + 1) // 2): "420"}.get(u.shape)
        if sub is None or v.shape != u.shape:
            raise ValueError("chroma planes {} / {} fit no subsampling of a {} x {} frame".format(u.shape, v.shape, W, H))
        S = self.view.size
        with ctx.slot_locks[slot]:
            bufs = [ctx.to_device(p, slot=slot) for p in (y, u, v)]
            dst = ctx.alloc(S * S * 3 * self.in_dtype.itemsize)
            try:
                self.convert_dev(ctx, [(bufs[0], bufs[1], bufs[2], W, H, sub, dst)], slot=slot)
                return ctx.download(dst, (S, S, 3), dtype=self.in_dtype, slot=slot)
            finally:
                for b in bufs + [dst]:
                    ctx.free(b)

    def close(self) -> None:
        if self._owns:
            self.color.close()
