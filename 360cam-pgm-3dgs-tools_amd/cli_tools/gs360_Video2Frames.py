#!/usr/bin/env python3
"""Drop-in for the reference's cli_tools/gs360_Video2Frames.py: a video -> an image sequence at N frames per second.

Flags, defaults, checks and their stderr messages, the default output folder `<stem>_frames_<fps>fps`, the file pattern
`<prefix>_%07d<suffix>.<ext>` from 0, the --overwrite rule, the `[exec]` line, the completion line and the exit codes are the
reference's (V2F:247-716).  What differs is where the pixels are made: ONE ffmpeg child decodes, cuts (-ss / -to / -map) and resamples
(fps=F) and pipes YUV4MPEG2; the colour conversion the reference asks of ffmpeg's `colorspace` filter (V2F:464-466) runs on the GPU
(gs360/vidcolor.py, VID-COLOR v1), and .jpg / .png frames are encoded from device memory when GS360_JPEG_ENCODER / GS360_PNG_ENCODER
say `device` (default `host`: gs360/imageio.py writes them, as it always writes .tif).

--fisheye-perspective (V2F:467-493: `v360=<fisheye|equisolid>:rectilinear:...:interp=cubic` before the colour filter, `scale=S:S`
after it) runs when GS360_V2F_FISHEYE=device: the decoder's command line stays as it is, and every frame leaves the GPU as the S x S
pinhole view of VID-FISHEYE v1 (gs360/vidfisheye.py, DESIGN.md section 18: the planes interpolated with v360's cubic, then converted;
rendered once at S x S, invisible pixels black; parity with a real ffmpeg's v360 is not pinned).  Without the variable the flag is
refused as before; any other value of it is an error.

Refused with one `[ERR]` line and exit code 1: --fisheye-perspective without GS360_V2F_FISHEYE=device, another value of that
variable, and a stream the Y4M reader refuses (12 bits and above, monochrome, interlaced, truncated).
"""
import argparse
import pathlib
import queue
import re
import shlex
import shutil
import subprocess
import sys
import threading

_HERE = pathlib.Path(__file__).resolve().parent
if str(_HERE.parent) not in sys.path:
    sys.path.insert(0, str(_HERE.parent))

FISHEYE_INPUT_FOV_DEG = 180.0
BATCH = 16                   # frames per conversion call (GS360_MAX_FRAMES)
IN_FLIGHT = 2 * BATCH        # decoded frames resident on the device at most
IMAGE_EXTS = ("jpg", "jpeg", "png", "tif", "tiff")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Extract frames from a video at N fps using ffmpeg.")
    ap.add_argument("-i", "-in", dest="video", required=True, help="Input video file path.")
    ap.add_argument("-o", "-out", dest="output", default=None, help="Output directory (defaults next to the input video).")
    ap.add_argument("-f", "--fps", type=float, required=True, help="Frame extraction rate in frames per second (e.g. 5, 2.5).")
    ap.add_argument("-e", "--ext", default="jpg", help="Output image extension (e.g. jpg, png). Defaults to jpg.")
    ap.add_argument("--prefix", default="out", help="Filename prefix for extracted frames (default: out).")
    ap.add_argument("--start", type=float, default=0.0, help="Optional start time in seconds.")
    ap.add_argument("--end", type=float, default=None, help="Optional end time in seconds.")
    ap.add_argument("--keep-rec709", action="store_true", help="Keep Rec.709 characteristics instead of converting to sRGB.")
    ap.add_argument("--overwrite", action="store_true", help="Overwrite output if it already exists.")
    ap.add_argument("--ffmpeg", default="ffmpeg", help="Path to the ffmpeg executable (default: ffmpeg).")
    ap.add_argument("--map-stream", dest="map_stream", default=None,
                    help="Optional ffmpeg -map argument (e.g. 0:v:0) to select a specific stream.")
    ap.add_argument("--name-suffix", dest="name_suffix", default="", help="Optional suffix inserted before the file extension (e.g. _X).")
    ap.add_argument("--fisheye-perspective", action="store_true",
                    help="Apply an experimental dual fisheye to perspective transform using ffmpeg v360 (intended for two fisheye streams).")
    ap.add_argument("--fisheye-focal-mm", type=float, default=8.0,
                    help="Focal length in millimetres for deriving perspective FOV when --fisheye-perspective is set (default: 8).")
    ap.add_argument("--fisheye-size", type=int, default=3840, help="Output square size in pixels for --fisheye-perspective (default: 3840).")
    ap.add_argument("--fisheye-projection", type=lambda value: value.lower(), choices=("equidistant", "equisolid"), default="equisolid",
                    help="Input fisheye projection model for --fisheye-perspective (equidistant or equisolid, default: equisolid).")
    ap.add_argument("--fisheye-input-fov", type=float, default=FISHEYE_INPUT_FOV_DEG,
                    help=f"Input fisheye field-of-view in degrees for --fisheye-perspective (default: {FISHEYE_INPUT_FOV_DEG:.0f}).")
    return ap


def fps_text(fps: float) -> str:
    """the fps as the default folder name carries it: 5.0 -> 5, 2.50 -> 2.5 (V2F:412-417)"""
    text = f"{fps}"
    return text.rstrip("0").rstrip(".") if "." in text else text


def _underscored(text: str) -> str:
    return re.sub(r"\s+", "_", text)


def output_layout(args, in_path: pathlib.Path):
    """-> (output folder, extension, prefix, suffix) by the reference's rules (V2F:411-441)"""
    if args.output:
        out_dir = pathlib.Path(args.output).expanduser().resolve()
    else:
        out_dir = in_path.parent / f"{in_path.stem}_frames_{fps_text(args.fps)}fps"
    prefix = _underscored((args.prefix or "out").strip()) or "out"
    suffix = _underscored(args.name_suffix.strip()) if args.name_suffix else ""
    return out_dir, args.ext.lstrip(".").lower(), prefix, suffix


def frame_path(out_dir, prefix, suffix, ext, k: int) -> pathlib.Path:
    return out_dir / f"{prefix}_{k:07d}{suffix}.{ext}"


def decoder_argv(args, ffmpeg_exec: str, in_path: pathlib.Path):
    """the one ffmpeg child: decode, cut, resample, pipe Y4M.  No colorspace filter, no RGB format: those are the GPU's."""
    cmd = [ffmpeg_exec, "-hide_banner"]
    if args.start is not None:
        cmd += ["-ss", str(args.start)]
    cmd += ["-i", str(in_path)]
    if args.end is not None:
        cmd += ["-to", str(args.end)]
    if args.map_stream:
        cmd += ["-map", args.map_stream]
    return cmd + ["-vf", f"fps={args.fps}", "-f", "yuv4mpegpipe", "-strict", "-1", "pipe:1"]


def _fail(text: str, code: int = 1) -> int:
    print(text, file=sys.stderr)
    return code


class _Frames:
    """Decoded frames on their way to the device: a reader thread fills pinned staging blocks from the pipe and uploads each frame's
    three planes, back to back, into one of IN_FLIGHT device buffers."""

    def __init__(self, ctx, reader, slot):
        self.ctx, self.reader, self.slot = ctx, reader, slot
        self.nbytes = reader.header.frame_bytes
        self.free = queue.Queue()
        self.ready = queue.Queue()
        self.error = None
        self.stop = threading.Event()
        self.buffers = []
        self.thread = threading.Thread(target=self._run, name="v2f-reader", daemon=True)
        self.thread.start()

    def _take(self):
        """a free device buffer: a new one while fewer than IN_FLIGHT exist, else the next one given back"""
        try:
            return self.free.get_nowait()
        except queue.Empty:
            if len(self.buffers) < IN_FLIGHT:
                self.buffers.append(self.ctx.alloc(self.nbytes + 64))
                return self.buffers[-1]
        while not self.stop.is_set():
            try:
                return self.free.get(timeout=0.1)
            except queue.Empty:
                continue
        return None

    def _run(self):
        import numpy as np
        staging = [self.ctx.pinned(self.nbytes) for _ in range(2)]
        try:
            k = 0
            while not self.stop.is_set():
                block = staging[k & 1]
                if not self.reader.read_into(block.view):
                    break
                buf = self._take()
                if buf is None:
                    break
                with self.ctx.slot_locks[self.slot]:
                    self.ctx.upload(buf, np.frombuffer(block.view, np.uint8, self.nbytes), slot=self.slot, sync=True)
                self.ready.put(buf)
                k += 1
        except Exception as exc:                   # a truncated frame, a failed upload: the main thread reports it
            self.error = exc
        finally:
            self.ready.put(None)
            for block in staging:
                self.ctx.unpin(block)

    def batches(self):
        """lists of up to BATCH device buffers, in stream order; whatever has arrived is taken without waiting for a full batch"""
        done = False
        while not done:
            batch = [self.ready.get()]
            while batch[-1] is not None and len(batch) < BATCH:
                try:
                    batch.append(self.ready.get_nowait())
                except queue.Empty:
                    break
            if batch[-1] is None:
                done = True
                batch.pop()
            if batch:
                yield batch

    def give_back(self, batch):
        for b in batch:
            self.free.put(b)

    def close(self):
        self.stop.set()
        self.thread.join(timeout=10)


def _plane_jobs(header, buf, dst):
    """the conversion job of a frame whose planes sit back to back in `buf`"""
    item = header.dtype.itemsize
    (h, w), (ch, cw), _ = header.plane_shapes
    y = buf.ptr
    cb = y + h * w * item
    cr = cb + ch * cw * item
    return (y, cb, cr, w, h, header.subsampling, dst)


def extract(args, ffmpeg_exec, in_path, out_dir, ext, prefix, suffix, fisheye=None) -> int:
    """fisheye: None, or the vidfisheye.FisheyeView every frame is rendered through"""
    import numpy as np
    import gs360
    from gs360 import imageio, jpegenc, pngenc, vidcolor, vidfisheye, y4m

    cmd = decoder_argv(args, ffmpeg_exec, in_path)
    print("\n[exec] " + " ".join(shlex.quote(x) for x in cmd) + "\n")
    proc = subprocess.Popen(cmd, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    tail = []

    def drain():
        for raw in proc.stderr:
            tail.append(raw.decode("utf-8", errors="replace").rstrip())
            del tail[:-20]
    drainer = threading.Thread(target=drain, name="v2f-stderr", daemon=True)
    drainer.start()

    def finish_decoder(kill=False):
        if kill and proc.poll() is None:
            proc.kill()
        proc.stdout.close()
        rc = proc.wait()
        drainer.join(timeout=5)
        return rc

    try:
        reader = y4m.Y4MReader(proc.stdout)
    except y4m.Y4MError as exc:
        try:
            rc = proc.wait(timeout=2)               # a decoder that failed has ended by itself
        except subprocess.TimeoutExpired:
            rc = 0
        finish_decoder(kill=True)
        if rc != 0:                                 # its exit code is the tool's (V2F:706-711)
            for line in tail[-5:]:
                print(line, file=sys.stderr)
            return _fail(f"ffmpeg execution failed (returncode={rc})", rc)
        return _fail(f"[ERR] {exc}")
    header = reader.header
    jpeg_mode = jpegenc.mode_from_env() if ext in ("jpg", "jpeg") else None
    png_device = pngenc.mode_from_env() if ext == "png" else False
    out_dtype = np.uint8 if header.depth == 8 else np.uint16          # V2F:462: 8 bits stay 8, anything deeper is written as 16
    H, W = (fisheye.size, fisheye.size) if fisheye else (header.height, header.width)       # of the frames written
    written = 0
    frames = None
    failure = None
    with gs360.Context(device=0, n_slots=2) as ctx:
        color = vidcolor.VideoColor(header.depth, header.full_range, args.keep_rec709)
        stage = vidfisheye.FisheyeStage(fisheye, header.depth, color=color) if fisheye else color
        dsts = []
        try:
            frames = _Frames(ctx, reader, slot=1)
            for batch in frames.batches():
                while len(dsts) < len(batch):
                    dsts.append(ctx.alloc(H * W * 3 * np.dtype(out_dtype).itemsize))
                with ctx.slot_locks[0]:
                    stage.convert_dev(ctx, [_plane_jobs(header, b, d) for b, d in zip(batch, dsts)], slot=0)
                paths = [frame_path(out_dir, prefix, suffix, ext, written + k) for k in range(len(batch))]
                if jpeg_mode is not None:
                    files = jpegenc.encode_device(ctx, [(d, H, W, 3) for d in dsts[:len(batch)]], quality=jpegenc.quality_for(1),
                                                  restart=jpegenc.RESTART, slot=0, huffman=jpeg_mode)
                elif png_device:
                    files = pngenc.encode_device(ctx, [(d, H, W, 3, np.dtype(out_dtype).itemsize, 0) for d in dsts[:len(batch)]], slot=0)
                else:
                    files = None
                    for p, d in zip(paths, dsts):
                        with ctx.slot_locks[0]:
                            rgb = ctx.download(d, (H, W, 3), dtype=out_dtype, slot=0)
                        imageio.write_image(p, rgb, jpeg_q=1)
                if files is not None:
                    ctx.sync(0)
                    for p, data in zip(paths, files):
                        p.write_bytes(data)
                frames.give_back(batch)
                written += len(batch)
                sys.stdout.write(f"\r[progress] frame {written}")
                sys.stdout.flush()
            failure = frames.error
        except (gs360.Gs360Error, imageio.ImageIOError, OSError) as exc:
            failure = exc
        finally:
            if frames is not None:
                frames.close()
            color.close()
    rc = finish_decoder(kill=failure is not None)
    if written:
        sys.stdout.write("\n")
        sys.stdout.flush()
    if failure is not None and not isinstance(failure, y4m.Y4MError):
        return _fail(f"[ERR] {failure}")
    if rc != 0:
        for line in tail[-5:]:
            print(line, file=sys.stderr)
        return _fail(f"ffmpeg execution failed (returncode={rc})", rc)
    if failure is not None:
        return _fail(f"[ERR] {failure}")
    print(f"Completed: {out_dir}")
    return 0


def run(argv=None) -> int:
    args = build_parser().parse_args(argv)
    ffmpeg_exec = args.ffmpeg or "ffmpeg"
    fisheye = None
    if not shutil.which(ffmpeg_exec):
        return _fail(f"ffmpeg executable not found: {ffmpeg_exec}")
    if args.fisheye_perspective:
        if args.fisheye_focal_mm <= 0.0:
            return _fail("Focal length must be greater than zero when using --fisheye-perspective.")
        if args.fisheye_size <= 0:
            return _fail("Output size must be greater than zero when using --fisheye-perspective.")
        if args.fisheye_input_fov <= 0.0:
            return _fail("Input fisheye FOV must be greater than zero when using --fisheye-perspective.")
        from gs360 import vidfisheye
        try:
            enabled = vidfisheye.mode_from_env()
        except ValueError as exc:
            return _fail(f"[ERR] {exc}")
        if not enabled:
            return _fail("[ERR] --fisheye-perspective is not implemented by this drop-in: the engine has no fisheye-input v360 remap yet")
        if args.fisheye_size > vidfisheye.MAX_SIDE:
            return _fail(f"[ERR] --fisheye-size {args.fisheye_size} is above the engine's {vidfisheye.MAX_SIDE}")
        fisheye = vidfisheye.view_from_args(args.fisheye_focal_mm, args.fisheye_size, args.fisheye_projection, args.fisheye_input_fov)
    in_path = pathlib.Path(args.video).expanduser().resolve()
    if not in_path.exists():
        return _fail(f"Input file not found: {in_path}")
    out_dir, ext, prefix, suffix = output_layout(args, in_path)
    if ext not in IMAGE_EXTS:
        return _fail(f"[ERR] unsupported output extension .{ext}: this drop-in writes {', '.join(IMAGE_EXTS)}")
    if out_dir.exists() and not out_dir.is_dir():
        return _fail(f"Output path exists and is not a directory: {out_dir}")
    out_dir.mkdir(parents=True, exist_ok=True)
    if not args.overwrite:
        existing = next(out_dir.glob(f"{prefix}_*{suffix}.{ext}"), None)
        if existing is not None:
            print(f"Output exists and overwrite is disabled. First match: {existing.name}", file=sys.stderr)
            return _fail("Enable --overwrite to replace existing frames.")
    return extract(args, ffmpeg_exec, in_path, out_dir, ext, prefix, suffix, fisheye)


def main() -> None:
    sys.exit(run())


if __name__ == "__main__":
    main()
