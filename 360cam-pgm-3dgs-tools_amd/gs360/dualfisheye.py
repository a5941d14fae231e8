"""GPU execution of the dual-fisheye pair pipeline (the per-pair work of DF:1910-2064).

One PairRenderer per device holds the remap tables of a sensor pair resident in HBM (the reference builds them
once per run and shares them between its worker threads, DF:2582-2592, DF:2776-2804) and renders all views of one
X/Y pair: upload the two lens images once, one table-remap launch per view (cv2.remap semantics + fused
`out[~valid] = mask_value`), download.  `fused=True` evaluates the map in-kernel instead (FE-SPEC v1, no table
traffic; <= 0.01 px from the reference tables).

The tables of a run never change, so pairs go through MAP PLANS (include/gs360.h): each table converted once to the fixed
point cv2.remap derives from it on every call, 5 bytes per pixel instead of 9 -- same results, less to read per pair.  Plans are made
on first use per (view, sampler class); sources beyond 4079 pixels keep the float tables.  GS360_MAP_PLANS=0
turns them off (A/B).

The reference writes every view with cv2.imwrite(path, image, [IMWRITE_JPEG_QUALITY, q]) (DF:1826-1840): libjpeg's defaults, 2 x 2 chroma
subsampling and the Annex K Huffman tables.  With GS360_JPEG_ENCODER=device (jpeg_mode_from_env, read once per run by the CLI) the 8-bit
.jpg views of a pair are entropy-coded where the remap left them ("JPG-SPEC v1, 4:2:0", gs360/jpegenc.py: one gs360_jpeg_scan_sub_u8
call on the pair's slot) and only the scans cross PCIe; render_pair then returns whole files instead of arrays.  GS360_PNG_ENCODER=device
(png_mode_from_env) does the same for the .png views and .png masks, 8- and 16-bit (PNG-SPEC v1, gs360/pngenc.py: one gs360_png_deflate
call), in place of cv2.imwrite's PNG writer.
"""
import os
import threading
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import capi, devcodec, jpegenc, pngenc
from .fisheye import SensorCalibration, UndistortTables

INTERPOLATIONS = {"nearest": 0, "linear": 1, "cubic": 2, "lanczos4": 4}   # cv2.INTER_* values (DF:59-64)


jpeg_mode_from_env = jpegenc.mode_from_env      # the CLI's name for it: read once per run
png_mode_from_env = pngenc.mode_from_env


def engine_interpolation(flag: int) -> int:
    """cv2 flag -> what the engine implements: all four of the tool's choices (nearest, linear, cubic, lanczos4)."""
    if flag not in (capi.INTERP_NEAREST, capi.INTERP_LINEAR, capi.INTERP_CUBIC, capi.INTERP_LANCZOS4):
        raise ValueError("unsupported interpolation flag {}".format(flag))
    return flag


class PairRenderer:
    def __init__(self, ctx: capi.Context, sensors: Dict[str, SensorCalibration], specs: Sequence[Dict[str, object]],
                 tables: Optional[Dict[str, Dict[str, object]]], undistort: Optional[Dict[str, UndistortTables]],
                 lens_fov_deg: float, fused: bool = False):
        self.ctx = ctx
        self.sensors = sensors
        self.specs = list(specs)
        self.tables = tables
        self.lens_fov_deg = float(lens_fov_deg)
        self.fused = bool(fused)
        self.lock = threading.Lock()       # one pair at a time per device context (slot 0)
        self.dev_tables = {}
        if tables and not fused:
            for vid, t in tables.items():
                self.dev_tables[vid] = (ctx.to_device(t["map_x"]), ctx.to_device(t["map_y"]),
                                        ctx.to_device(np.ascontiguousarray(t["valid"], np.uint8)))
        self._scratch = None                # grow-only output buffer shared by the per-view launches of a pair
        self._plans = {}                    # (kind, id, nearest) -> map plan handle
        self.use_plans = os.environ.get("GS360_MAP_PLANS", "1") not in ("0", "off", "no")
        self._stats = {"jpeg_device_images": 0, "jpeg_device_bytes": 0, "png_device_images": 0, "png_device_bytes": 0}
        self.dev_undistort = {}
        for sid, u in (undistort or {}).items():
            self.dev_undistort[sid] = (ctx.to_device(u.map_x), ctx.to_device(u.map_y),
                                       ctx.to_device(np.ascontiguousarray(u.valid_mask, np.uint8)))

    # ---------------------------------------------------------------------------------------------
    def _plan(self, kind, key, maps, out_hw, interp, shape, dtype):
        """-> the map plan for these tables and this sampler class, or None where plans do not apply"""
        H, W = shape[0], shape[1]
        if not self.use_plans or max(H, W) > self.ctx.MAP_PLAN_MAX_DIM:
            return None
        nearest = interp == capi.INTERP_NEAREST
        k = (kind, key, nearest)
        if k not in self._plans:
            self._plans[k] = self.ctx.map_plan(maps[0], maps[1], maps[2], out_hw[0], out_hw[1], nearest=nearest, slot=0)
        return self._plans[k]

    def stats(self):
        """jpeg_device_images / jpeg_device_bytes: views the device encoder wrote (render_pair's jpeg_views / jpeg_masks) and their
        files' bytes, as Engine.stats() counts them"""
        with self.lock:
            return {k: v for k, v in self._stats.items() if k.startswith("jpeg")}

    def png_stats(self):
        """png_device_images / png_device_bytes: the same counts for the device PNG encoder (render_pair's png_views / png_masks)"""
        with self.lock:
            return {k: v for k, v in self._stats.items() if k.startswith("png")}

    def _collect(self, keys, bufs, shapes, dtype, encoder):
        """(the views' launch queued on slot 0) -> {key: array}, or with `encoder` = (quality, huffman) and 8-bit gray or
        RGB views {key: bytes}: whole 4:2:0 JFIF files, encoded from the device buffers before they are freed.  A scan gets the view's
        raw size; one that needs more is coded again, in the same mode, into a buffer of the bound.  `encoder` a devcodec.PngMode: whole
        PNG files in the same way, for views of either depth and 1, 3 or 4 channels."""
        png = isinstance(encoder, devcodec.PngMode)
        if encoder is None or not (png or (np.dtype(dtype) == np.uint8 and all(c in (1, 3) for _h, _w, c in shapes))):
            return {k: self.ctx.download(b, shape, dtype=dtype, slot=0) for k, b, shape in zip(keys, bufs, shapes)}
        with self.ctx.slot_locks[0]:
            if png:
                esz = np.dtype(dtype).itemsize
                files = pngenc.encode_buffers(self.ctx, [(b, h, w, c, esz, 0) for b, (h, w, c) in zip(bufs, shapes)], slot=0, raw_capacity=True)
            else:
                quality, huffman = encoder
                files = jpegenc.encode_buffers(self.ctx, [(b, h, w, c) for b, (h, w, c) in zip(bufs, shapes)], quality=int(quality),
                                               restart=jpegenc.RESTART, slot=0, huffman=huffman, subsampling="4:2:0", raw_capacity=True)
        self._stats["png_device_images" if png else "jpeg_device_images"] += len(files)
        self._stats["png_device_bytes" if png else "jpeg_device_bytes"] += sum(len(f) for f in files)
        return dict(zip(keys, files))

    def close(self):
        """release the plans (the context's own close releases everything else)"""
        with self.lock:
            for plan in self._plans.values():
                if self.ctx.handle:
                    self.ctx.map_plan_free(plan)
            self._plans.clear()

    def _remap(self, d_src, shape, maps, out_hw, interp, border, valid_fill, dtype=np.uint8, plan_key=None):
        H, W, C = shape
        h, w = out_hw
        need = h * w * C * np.dtype(dtype).itemsize
        if self._scratch is None or self._scratch.nbytes < need:
            if self._scratch is not None:
                self.ctx.free(self._scratch)
            self._scratch = self.ctx.alloc(need)
        plan = self._plan("undistort", plan_key, maps, out_hw, interp, shape, dtype) if plan_key is not None else None
        if plan is not None:
            self.ctx.remap_plans_dev([(d_src, H, W, plan, valid_fill is not None, h, w, valid_fill if valid_fill is not None else 0,
                                       self._scratch)], C, interp=interp, border_value=border, slot=0, dtype=dtype)
        else:
            self.ctx.remap_table_dev(d_src, H, W, C, maps[0], maps[1], maps[2] if valid_fill is not None else None, h, w,
                                     self._scratch, interp=interp, border_value=border,
                                     fill_value=valid_fill if valid_fill is not None else 0, slot=0, dtype=dtype)
        return self.ctx.download(self._scratch, (h, w, C), dtype=dtype, slot=0)

    def _remap_views(self, dev, imgs, dmask, interp, border, valid_fill, encoder=None):
        """All views of the pair in ONE batched launch (no per-view launch tails), then the downloads (or, with `encoder`, the device
        encoder: _collect).  `dmask` set: the per-lens mask images are the sources (DF:2031-2043), else the lens images."""
        dtype = np.uint8
        if dmask is None and any(v.dtype == np.uint16 for v in imgs.values()):
            if any(v.dtype != np.uint16 for v in imgs.values()):
                raise RuntimeError("the two lens images differ in bit depth")
            dtype = np.uint16                 # CV_16U samplers, the same batched launch (gs360_remap_tables_u16)
        esz = np.dtype(dtype).itemsize
        jobs, shapes, bufs, planned = [], [], [], []
        for spec in self.specs:
            vid = str(spec["view_id"])
            key = self.tables[vid]["lens_key"]
            if dmask is not None:
                if key not in dmask:
                    raise RuntimeError("Mask source missing for lens {}".format(key))
                d_src, (H, W, C) = dmask[key]
            else:
                d_src, (H, W, C) = dev[key], imgs[key].shape
            h, w = int(spec["height"]), int(spec["width"])
            d_dst = self.ctx.alloc(h * w * C * esz)
            bufs.append(d_dst)
            mx, my, va = self.dev_tables[vid]
            jobs.append((d_src, H, W, mx, my, va if valid_fill is not None else None, h, w,
                         valid_fill if valid_fill is not None else 0, d_dst))
            plan = self._plan("view", vid, (mx, my, va), (h, w), interp, (H, W, C), dtype)
            planned.append(None if plan is None else (d_src, H, W, plan, valid_fill is not None, h, w,
                                                      valid_fill if valid_fill is not None else 0, d_dst))
            shapes.append((vid, (h, w, C)))
        try:
            channels = {s[1][2] for s in shapes}
            if len(channels) != 1:
                raise RuntimeError("the two lens images differ in channel count")
            if all(p is not None for p in planned):
                self.ctx.remap_plans_dev(planned, channels.pop(), interp=interp, border_value=border, slot=0, dtype=dtype)
            else:
                self.ctx.remap_tables_dev(jobs, channels.pop(), interp=interp, border_value=border, slot=0, dtype=dtype)
            return self._collect([vid for vid, _s in shapes], bufs, [shape for _v, shape in shapes], dtype, encoder)
        finally:
            for b in bufs:
                self.ctx.free(b)

    def render_pair(self, image_x: np.ndarray, image_y: np.ndarray, sensor_id_x: str, sensor_id_y: str, *,
                    interpolation: int, mask_outside_model: bool, mask_value: int,
                    mask_x: Optional[np.ndarray] = None, mask_y: Optional[np.ndarray] = None,
                    want_fisheye: bool = False, want_perspective: bool = True,
                    color_stage=None, want_color: bool = False, jpeg_views=None, jpeg_masks=None, png_views: bool = False,
                    png_masks: bool = False):
        """-> dict(perspective={view_id: img}, masks={view_id: img}, fisheye={'X': img, 'Y': img}, color={'X','Y'})

        `jpeg_views` = None | (quality, huffman): when set and the views are 8-bit with C = 1 or 3, the perspective entries are not
        downloaded: the batch's device buffers go into one gs360_jpeg_scan_sub_u8(..., GS360_JPEG_420, ...) call on the same slot and
        every entry is a whole JFIF file (bytes: header + scan + EOI), what cv2.imwrite writes at DF:1826-1840 up to the DCT's rounding.
        `jpeg_masks`: the same for the mask entries, whose files carry their own extension (--perspective-mask-ext).  16-bit and
        four-channel views, the undistorted-fisheye and the colour-corrected outputs stay arrays.
        `png_views` / `png_masks`: the perspective / mask entries are whole PNG files from the device encoder (gs360_png_deflate; any
        depth and channel count), in place of `jpeg_views` / `jpeg_masks`.

        `color_stage` (gs360.color.ColorStage) converts both lens images on the device right after the upload, i.e.
        before every resampling step, as load_prepared_input_image does on the host (DF:728-743); `want_color`
        returns the converted images (the --save-color-corrected-output files, DF:1953-1959)."""
        interp = engine_interpolation(interpolation)
        view_mode = devcodec.PngMode() if png_views else jpeg_views
        mask_mode = devcodec.PngMode() if png_masks else jpeg_masks
        out = {"perspective": {}, "masks": {}, "fisheye": {}, "color": {}}
        with self.lock:
            imgs = {"X": _hwc(image_x), "Y": _hwc(image_y)}
            dev = {k: v.buf for k, v in imgs.items() if isinstance(v, DeviceImage)}      # (freed below with the uploads)
            try:
                if color_stage is not None:
                    for v in imgs.values():
                        color_stage.check_image(v.shape, v.dtype)
                for k, v in imgs.items():
                    if k not in dev:
                        dev[k] = self.ctx.to_device(v)
            except Exception:
                for b in dev.values():
                    self.ctx.free(b)
                raise
            dmask = {}
            for k, m in (("X", mask_x), ("Y", mask_y)):
                if m is not None:
                    dmask[k] = (self.ctx.to_device(_hwc(m)), _hwc(m).shape)
            try:
                if color_stage is not None:
                    for k, v in imgs.items():
                        color_stage.apply_dev(self.ctx, dev[k], v.shape, red_index=0, slot=0, dtype=v.dtype)   # arrays here are RGB(A)
                if want_color:
                    for k, v in imgs.items():
                        on_device = color_stage is not None or isinstance(v, DeviceImage)
                        out["color"][k] = self.ctx.download(dev[k], v.shape, dtype=v.dtype, slot=0) if on_device else v
                # borderValue=float(mask_value) -> cv::Scalar(v,0,0,0): only channel 0 gets v, and channel 0 of a
                # cv2.imread image is BLUE.  Arrays here are RGB(A), so the value goes to index 2 for colour images.
                C_in = imgs["X"].shape[2]
                border = (0.0, 0.0, float(mask_value), 0.0) if C_in >= 3 else (float(mask_value), 0.0, 0.0, 0.0)
                fill = int(mask_value) if mask_outside_model else None
                if want_fisheye:
                    for key, sid in (("X", sensor_id_x), ("Y", sensor_id_y)):
                        c = self.sensors[sid]
                        if imgs[key].shape[:2] != (c.height, c.width):
                            raise RuntimeError("Resolution mismatch for {} lens: got {}x{}, expected {}x{}".format(
                                key, imgs[key].shape[1], imgs[key].shape[0], c.width, c.height))
                        out["fisheye"][key] = self._remap(dev[key], imgs[key].shape, self.dev_undistort[sid],
                                                          (c.height, c.width), interp, border, fill, dtype=imgs[key].dtype, plan_key=sid)
                if want_perspective:
                    if self.fused and imgs["X"].dtype == np.uint16:
                        raise RuntimeError("16-bit lens images need table mode (the fused-map kernel is 8-bit)")
                    if self.fused:
                        self._render_fused(out, imgs, dev, sensor_id_x, sensor_id_y, interp, mask_outside_model, mask_value, border, view_mode)
                    else:
                        out["perspective"] = self._remap_views(dev, imgs, None, interp, border, fill, view_mode)
                    if dmask:
                        if self.fused:   # masks always go through the table path (nearest, border 0, invalid -> 0)
                            raise RuntimeError("mask rendering needs table mode")
                        out["masks"] = self._remap_views(None, None, dmask, capi.INTERP_NEAREST, (0.0, 0.0, 0.0, 0.0),
                                                         0 if mask_outside_model else None, mask_mode)
            finally:
                for b in dev.values():
                    self.ctx.free(b)
                for b, _s in dmask.values():
                    self.ctx.free(b)
        return out

    def _render_fused(self, out, imgs, dev, sid_x, sid_y, interp, mask_outside, mask_value, border, encoder=None):
        views, calibs, srcs, dsts = [], [], [], []
        C = imgs["X"].shape[2]
        for key, sid in (("X", sid_x), ("Y", sid_y)):
            c = self.sensors[sid]
            if imgs[key].shape[:2] != (c.height, c.width):
                raise RuntimeError("fused map mode needs images of the calibrated size {}x{} (lens {} is {}x{})".format(
                    c.width, c.height, key, imgs[key].shape[1], imgs[key].shape[0]))
        for spec in self.specs:
            vid = str(spec["view_id"])
            t = self.tables[vid]
            key = t["lens_key"]
            c = self.sensors[sid_x if key == "X" else sid_y]
            views.append(capi.View.make(t["yaw_rel_deg"], spec["pitch_deg"], spec["hfov_deg"], spec["vfov_deg"],
                                        spec["width"], spec["height"]))
            calibs.append(capi.Calib.make(c.width, c.height, c.f, c.cx, c.cy, c.k1, c.k2, c.k3, c.k4, c.p1, c.p2, c.b1, c.b2))
            srcs.append(dev[key])
            dsts.append(self.ctx.alloc(int(spec["width"]) * int(spec["height"]) * C))
        try:
            self.ctx.fisheye_views_dev(srcs, calibs, C, views, self.lens_fov_deg, dsts, interp=interp,
                                       mask_outside=mask_outside, mask_value=mask_value, slot=0, border_value=border)
            out["perspective"] = self._collect([str(spec["view_id"]) for spec in self.specs], dsts,
                                               [(int(spec["height"]), int(spec["width"]), C) for spec in self.specs], np.uint8, encoder)
        finally:
            for d in dsts:
                self.ctx.free(d)


class DeviceImage:
    """An 8-bit H x W x C lens image that is in device memory already (gs360.jpegdec with GS360_JPEG_DECODER=device): render_pair
    takes it in place of an array, uses the buffer as the uploaded image and frees it."""
    ndim = 3

    def __init__(self, buf, shape):
        self.buf, self.shape, self.dtype = buf, tuple(int(v) for v in shape), np.dtype(np.uint8)


def _hwc(a: np.ndarray) -> np.ndarray:
    """uint8 stays uint8; uint16 sources (cv2.imread(IMREAD_UNCHANGED), DF:735) stay uint16"""
    if isinstance(a, DeviceImage):
        return a
    a = np.ascontiguousarray(a, dtype=np.uint16 if np.asarray(a).dtype == np.uint16 else np.uint8)
    return a if a.ndim == 3 else a[:, :, None]
