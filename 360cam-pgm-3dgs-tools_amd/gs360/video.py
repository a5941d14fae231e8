"""Video inputs: ONE decode per video, frames resident in HBM, every view job samples the resident frames.

The reference plans one ffmpeg process per (video, view) (PC:830-836); each of those decodes the whole video again and
runs v360 on one thread ("N_views single-thread ffmpeg procs, each re-decoding the input").  Here the
first view job of a video starts a single decoder process -- the job's own ffmpeg command line with the v360 filter and
the encoder options removed and `format=rgb24 ... -f image2pipe -c:v ppm pipe:1` appended -- and a reader thread
uploads every frame to device memory through two pinned staging blocks per device (the pipe read of one frame overlaps
the H2D copy of the previous one; frames are dealt round-robin over the visible GPUs, so all views of a frame share a
device and there is no exchange step).  An 8K RGB frame is 88.5 MB: a 288 GB MI355X keeps > 2000 of them, i.e. the
whole 600-frame workload of BASELINE config 3 stays resident while the 12 view jobs run over it.  Longer videos stream:
past the budget (GS360_VIDEO_CACHE_GB per device) the frames every registered view job has consumed are retired and the
reader waits for the view jobs instead of failing (ffmpeg itself streams, PC:318, PC:746-749).

Two argv shapes are understood (anything else returns None and the caller falls back to the reference's subprocess):
  * the planner's:        -ss S -i V -to T -vf fps=F,colorspace=...,v360=... -vsync vfr -start_number 0 ... out_%07d_X.png
  * the GUI's selection:  -copyts -i V -ss S -to T -vf select='eq(n\\,i)+...',colorspace=...,v360=... -frame_pts 1 ...
    (gs360_GUI.py:19081-19148): output numbers are the selected source frame indices.
With GS360_VIDEO_FEED=planes (VID-FEED v1) the decoder only decodes: the job's colorspace= filter, one of the
reference's forms, leaves its command line, it pipes YUV4MPEG2 planes (half the bytes of the RGB frame), and gs360/vidcolor.py
converts them into the resident RGB frame on the upload stream; a stream header the conversion does not take restarts the decoder
once on the PPM command.
Geometry/sampling are the engine's (EQ-SPEC v1 on RGB); ffmpeg's v360 interpolates the YUV planes, so outputs are not
bit-comparable with the reference's -- parity at this seam is unpinned (no ffmpeg in the build or test images).
"""
import os
import re
import subprocess
import time
import tempfile
import threading
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import capi, y4m
from .jobspec import JobSpec
from .vidcolor import VideoColor

# options that belong to the encoder / muxer of the per-view process and have no meaning for the shared decoder
_ENCODER_OPTIONS = {"-c:v", "-q:v", "-qmin", "-qmax", "-pix_fmt", "-huffman", "-colorspace", "-color_primaries",
                    "-color_trc", "-start_number", "-frame_pts", "-threads", "-frames:v", "-loglevel"}
_DECODER_OPTIONS = {"-ss", "-to", "-t", "-vsync", "-fps_mode", "-r"}
_BUDGET_BYTES = int(float(os.environ.get("GS360_VIDEO_CACHE_GB", "200")) * (1 << 30))
_EVENT_BASE = 6                            # HIP events 6 / 7 of the upload slot mark the two staging blocks' copies


@dataclass(frozen=True)
class DecodePlan:
    argv: Tuple[str, ...]                 # the decoder command line
    key: Tuple                            # identical for every view job of the same video + decode settings
    numbers: Optional[Tuple[int, ...]]    # output number of the k-th decoded frame; None = start_number + k
    start_number: int
    feed: str = "ppm"                     # "ppm": RGB frames from the decoder; "planes": Y4M planes, converted on the device
    keep_rec709: bool = False             # planes: the removed colorspace filter had no trc option (the Rec.709 curve stays)
    out_bits: int = 8                     # planes: depth of the resident RGB frames (16 for -pix_fmt rgb48le)
    fallback_argv: Tuple[str, ...] = ()   # planes: the PPM command the reader restarts on when the stream's header is not convertible


FEED_ENV = "GS360_VIDEO_FEED"
_CS_REQUIRED = {"iall=bt709", "all=smpte170m", "format=yuv444p"}
_CS_OPTIONAL = {"trc=iec61966-2-1", "range=jpeg"}


def feed_from_env(environ=None) -> str:
    """GS360_VIDEO_FEED: unset, empty or `ppm` -> "ppm", `planes` -> "planes" (VID-FEED v1), anything else is an error"""
    value = (os.environ if environ is None else environ).get(FEED_ENV, "")
    if value in ("", "ppm"):
        return "ppm"
    if value == "planes":
        return "planes"
    raise ValueError("{} must be `ppm`, `planes` or unset (got {!r})".format(FEED_ENV, value))


def _reference_colorspace(flt: str) -> Optional[bool]:
    """One of the reference's colorspace= forms (PC:299-314: iall=bt709, all=smpte170m, format=yuv444p, optionally trc=iec61966-2-1,
    optionally range=jpeg, in any order) -> its keep_rec709 ("no trc option"); None for any other option set."""
    opts = flt[len("colorspace="):].split(":")
    have = set(opts)
    if len(have) != len(opts) or not _CS_REQUIRED <= have or have - _CS_REQUIRED - _CS_OPTIONAL:
        return None
    return "trc=iec61966-2-1" not in have


def _select_indices(flt: str) -> Optional[List[int]]:
    """select='eq(n\\,3)+eq(n\\,17)' -> [3, 17]; None when the expression is anything else."""
    body = flt[len("select="):].strip()
    if len(body) >= 2 and body[0] == "'" and body[-1] == "'":
        body = body[1:-1]
    out = []
    for clause in body.split("+"):
        m = re.fullmatch(r"eq\(n\\?,(\d+)\)", clause.strip())
        if not m:
            return None
        out.append(int(m.group(1)))
    return out


def build_decode_plan(job: JobSpec, feed: str = "ppm") -> Optional[DecodePlan]:
    """Decoder command for a video view job, or None when the argv is not one of the two understood shapes.  feed "planes" (VID-FEED
    v1): the chain's one colorspace= filter, when it is one of the reference's forms, is taken out of the
    decoder's chain and the decoder writes Y4M planes; any other chain keeps the PPM plan."""
    if feed not in ("ppm", "planes"):
        raise ValueError("feed must be `ppm` or `planes` (got {!r})".format(feed))
    if job.is_still_image or job.filters_after:
        return None
    if "%" not in job.dst.name:
        return None
    pix = job.options.get("-pix_fmt", "")
    if pix and pix not in ("rgb24", "yuvj444p", "rgb48le"):
        return None
    deep = pix == "rgb48le"                # bit depth > 8 (PC:343-347): frames travel as 16-bit PPM, views are uint16
    known = _ENCODER_OPTIONS | _DECODER_OPTIONS
    for tok in job.input_options[0::2] + job.output_options[0::2]:
        if tok not in known:
            return None
    numbers = None
    pre = [f for f in job.filters if f not in job.filters_after]
    for f in pre:
        if f.startswith("select="):
            idx = _select_indices(f)
            if idx is None:
                return None
            numbers = tuple(sorted(set(idx)))
    if numbers is not None and job.options.get("-frame_pts") != "1":
        numbers = None                     # select without frame_pts: plain sequential numbering
    if numbers is None and "-frame_pts" in job.options:
        return None                        # pts-driven numbering without a select list cannot be reproduced
    if numbers is not None and any(k in job.options for k in ("-ss", "-to", "-t")):
        # The GUI keeps -ss/-to on the OUTPUT side next to -copyts (gs360_GUI.py:19094-19148): ffmpeg then drops every
        # selected frame whose timestamp lies outside [S, T], and -frame_pts still names the survivors by their own
        # index.  The PPM pipe carries no timestamps, so which selected indices survive cannot be known here without
        # probing the stream; pairing the k-th decoded frame with the k-th selected index would misnumber every output.
        # Such jobs stay on the reference's per-view subprocess path.
        return None
    argv = [job.program, "-hide_banner", "-loglevel", "error", "-nostdin"]
    argv += [f for f in job.flags if f == "-copyts"]

    def keep(tokens: Sequence[str]) -> List[str]:
        out = []
        for k, v in zip(tokens[0::2], tokens[1::2]):
            if k in _DECODER_OPTIONS:
                out += [k, v]
        return out
    argv += keep(job.input_options) + ["-i", str(job.src)] + keep(job.output_options)
    head = list(argv)
    argv += ["-vf", ",".join(pre + ["format=rgb48be" if deep else "format=rgb24"]), "-an", "-f", "image2pipe", "-c:v", "ppm", "pipe:1"]
    start = int(job.options.get("-start_number", "0")) if numbers is None else 0
    if feed == "planes":
        cs = [f for f in pre if f.startswith("colorspace=")]
        keep_rec709 = _reference_colorspace(cs[0]) if len(cs) == 1 else None
        if keep_rec709 is not None:
            rest = [f for f in pre if f is not cs[0]]
            y4m_argv = head + ["-vf", ",".join(rest) if rest else "null", "-an", "-f", "yuv4mpegpipe", "-strict", "-1", "pipe:1"]
            out_bits = 16 if deep else 8
            # the colour options left the command line: they are part of what view jobs must agree on to share a decode
            key = (str(job.src), tuple(y4m_argv[1:]), keep_rec709, out_bits)
            return DecodePlan(tuple(y4m_argv), key, numbers, start, "planes", keep_rec709, out_bits, tuple(argv))
    key = (str(job.src), tuple(argv[1:]))
    return DecodePlan(tuple(argv), key, numbers, start)


def output_path(job: JobSpec, plan: DecodePlan, k: int) -> str:
    n = plan.numbers[k] if plan.numbers is not None and k < len(plan.numbers) else plan.start_number + k
    return str(job.dst) % n


# ---- PPM stream ------------------------------------------------------------------------------------------------
class PpmError(RuntimeError):
    pass


def read_ppm_header(stream) -> Optional[Tuple[int, int, int]]:
    """Reads one binary-PPM header from a buffered byte stream -> (width, height, maxval), None at a clean EOF."""
    tokens, cur, in_comment = [], b"", False
    while len(tokens) < 4:
        ch = stream.read(1)
        if not ch:
            if not tokens and not cur:
                return None
            raise PpmError("truncated PPM header")
        if in_comment:
            in_comment = ch != b"\n"
            continue
        if ch == b"#":
            in_comment = True
        elif ch.isspace():
            if cur:
                tokens.append(cur)
                cur = b""
        else:
            cur += ch
            if len(cur) > 16:
                raise PpmError("not a PPM stream")
    if tokens[0] != b"P6":
        raise PpmError("expected a binary PPM (P6) frame, got {!r}".format(tokens[0][:8]))
    try:
        w, h, maxval = (int(t) for t in tokens[1:])
    except ValueError as exc:
        raise PpmError("bad PPM header") from exc
    if w < 1 or h < 1 or w > 65535 or h > 65535 or maxval < 1 or maxval > 65535:
        raise PpmError("bad PPM geometry {}x{} maxval {}".format(w, h, maxval))
    return w, h, maxval


def read_exact_into(stream, mv: memoryview) -> None:
    got = 0
    while got < len(mv):
        n = stream.readinto(mv[got:])
        if not n:
            raise PpmError("truncated PPM frame ({} of {} bytes)".format(got, len(mv)))
        got += n


# ---- session ---------------------------------------------------------------------------------------------------
class SharedBudget:
    """Device memory all live sessions of one engine may hold together (GS360_VIDEO_CACHE_GB per device x devices).  A session
    superseded by a second decode of the same video stays alive until its last job leaves; with a budget of its own each, two
    sessions could ask for twice the budget of a device."""

    def __init__(self, total):
        self.total = int(total)
        self.used = 0
        self.lock = threading.Lock()

    def add(self, n):
        with self.lock:
            self.used += n


class FeedStats:
    """what an engine's sessions did with `planes` plans, summed (Engine.video_feed_stats)"""

    def __init__(self):
        self.plane_fed_frames = 0
        self.feed_fallbacks = 0
        self.lock = threading.Lock()

    def add(self, frames, fallbacks):
        with self.lock:
            self.plane_fed_frames += frames
            self.feed_fallbacks += fallbacks


# View jobs take the frames of a video in WINDOWS of this many (one batched launch per window and device: ring families -- the
# `full360coverage` preset, PC:616-680 -- reach the source-major kernel from four frames per call, csrc/gs360_capi_equirect.hip); frames are dealt to
# the devices in blocks of a window, so that a window's frames sit on one device.  GS360_VIDEO_WINDOW=1: one frame per launch (A/B).
_WINDOW = max(1, min(16, int(os.environ.get("GS360_VIDEO_WINDOW", "4"))))
_WINDOW_WAIT_S = 0.05                             # longest a view job waits for the frames behind the first one of its window


class VideoSession:
    """Decoded frames of one video on the engine's devices, streamed: the reader keeps at most `budget` bytes resident, view
    jobs walk the frames with a cursor each, and a frame every registered job has passed is retired when the reader needs
    the room (before that it stays, so that a view job that joins later still finds the video from its first frame).  The
    reader blocks -- back-pressure on the decoder's pipe -- while nothing can be retired.  A job that arrives after frames
    were retired cannot join (join() returns None): the engine starts a second session for it and its fellow late-comers.
    Thread-safe."""

    def __init__(self, states, plan: DecodePlan, stop_event=None, register_proc=None, budget=None, shared=None, feed_stats=None):
        self.states = states
        self.plan = plan
        self.stop_event = stop_event
        self.register_proc = register_proc       # callable(proc, add: bool): lets the caller's cancel handler see the decoder
        per_device = _BUDGET_BYTES if budget is None else budget
        self.budget = per_device * max(1, len(states))    # the budget is per device; frames are dealt round-robin
        self.shared = shared if shared is not None else SharedBudget(self.budget)   # `shared`: the engine's, one for all sessions
        self.frames = {}                          # k -> (state, DeviceBuffer, H, W, dtype), k in [first, count)
        self.first = 0                            # frames below `first` have been retired
        self.count = 0                            # frames published so far
        self.bytes = 0
        self.peak_bytes = 0
        self.retired = 0
        self.finished = False
        self.error: Optional[str] = None
        self.cond = threading.Condition()
        self.cursors = {}                         # job token -> index of the frame the job is working on (all below are done)
        self._next_token = 0
        self.active_jobs = 0
        self.done_jobs = 0
        self.closing = False
        self.proc = None
        self.color = None                         # `planes` feed: the session's VideoColor (a plan per device context), closed with it
        self.plane_fed_frames = 0                 # frames converted from planes on the device
        self.feed_fallbacks = 0                   # 1 when a `planes` plan went back to its PPM command at the stream header
        self.feed_stats = feed_stats              # the engine's FeedStats, or None
        self.thread = threading.Thread(target=self._reader, name="gs360-video-decode", daemon=True)
        self.thread.start()

    # reader thread ---------------------------------------------------------------------------------------------
    def _make_room(self, nbytes):
        """Called by the reader with self.cond held: retire passed frames until `nbytes` more fit, waiting for the view jobs
        to advance when nothing can go.  A single frame larger than the whole budget is admitted alone."""
        while self.shared.used + nbytes > self.shared.total and self.bytes > 0:
            if not self._retire_one():
                if self.closing or (self.stop_event is not None and self.stop_event.is_set()):
                    raise PpmError("cancelled")
                self.cond.wait(timeout=0.25)

    def _retire_one(self) -> bool:
        """(self.cond held) free the oldest frame if every registered job has passed it"""
        low = min(self.cursors.values()) if self.cursors else self.first      # no job registered: nothing has been passed
        if self.first >= low or self.first not in self.frames:
            return False
        st, buf, h, w, dt = self.frames.pop(self.first)
        n = h * w * 3 * np.dtype(dt).itemsize
        self.bytes -= n
        self.shared.add(-n)
        self.first += 1
        self.retired += 1
        if st.ctx.handle:
            st.ctx.free(buf)
        return True

    def _alloc(self, st, nbytes):
        """device block for the next frame; when the device itself is out of memory (other users of the GPU, a budget set too
        high) the reader does what it does at the budget: retire a passed frame, or wait for the view jobs, and try again"""
        while True:
            try:
                return st.ctx.alloc(nbytes)
            except capi.Gs360Error as exc:
                if exc.code != -5:
                    raise
                with self.cond:
                    if self.bytes == 0:
                        raise                     # nothing of ours to give back: the frame does not fit at all
                    if not self._retire_one():
                        if self.closing or (self.stop_event is not None and self.stop_event.is_set()):
                            raise PpmError("cancelled") from exc
                        self.cond.wait(timeout=0.25)

    def _publish(self, st, buf, h, w, fdtype, nbytes):
        with self.cond:
            self.frames[self.count] = (st, buf, h, w, fdtype)
            self.count += 1
            self.bytes += nbytes
            self.shared.add(nbytes)
            self.peak_bytes = max(self.peak_bytes, self.bytes)
            self.cond.notify_all()

    def _start_decoder(self, argv, errlog):
        try:
            self.proc = subprocess.Popen(list(argv), stdout=subprocess.PIPE, stderr=errlog, bufsize=1 << 20)
        except OSError as exc:
            raise PpmError("{}: {}".format(argv[0], exc)) from exc
        if self.register_proc:
            self.register_proc(self.proc, True)
        return self.proc.stdout

    def _open_planes(self, out):
        """The Y4M reader of a `planes` decoder, or None when the reader has to go back to the PPM feed: the header is not 8- or
        10-bit progressive 4:2:0 / 4:2:2 / 4:4:4, or it is 8-bit where 16-bit frames were asked for (the PPM path widens those as
        the reference's format filter does)."""
        try:
            reader = y4m.Y4MReader(out)
        except y4m.Y4MError:
            return None
        if reader.header.depth == 8 and self.plan.out_bits == 16:
            return None
        return reader

    def _fall_back(self, errlog):
        """kill and reap the `planes` decoder, start the plan's PPM command: once, before any frame is published"""
        proc = self.proc
        try:
            proc.kill()
        except Exception:
            pass
        proc.wait()
        proc.stdout.close()
        if self.register_proc:
            self.register_proc(proc, False)
        errlog.seek(0)
        errlog.truncate()
        self.feed_fallbacks += 1
        if self.feed_stats is not None:
            self.feed_stats.add(0, 1)
        out = self._start_decoder(self.plan.fallback_argv, errlog)
        if self.closing:                          # close() may have killed the decoder this one replaces
            raise PpmError("cancelled")
        return out

    def _reader(self):
        pinned = {}                               # (device, nbytes) -> [two pinned blocks]
        blocks = {}                               # (device, frame_bytes) -> (state, [two device plane blocks]), `planes` feed only
        turn = {}                                 # device -> which of its two blocks the next frame takes
        pending = None                            # (state, event index, publish args) of the upload still in flight
        errlog = None
        try:
            # stderr goes to an unnamed temporary file, not a pipe: a damaged stream can make ffmpeg print more than a pipe
            # buffer holds while this thread is blocked on stdout, which would stall decoder and view jobs alike
            errlog = tempfile.TemporaryFile()
            out = self._start_decoder(self.plan.argv, errlog)
            reader = None                         # `planes` feed: the Y4M stream; None = PPM frames
            if self.plan.feed == "planes":
                reader = self._open_planes(out)
                if reader is None:
                    out = self._fall_back(errlog)
                else:
                    hd = reader.header
                    self.color = VideoColor(hd.depth, hd.full_range, self.plan.keep_rec709, out_bits=8 if hd.depth == 8 else self.plan.out_bits)
            k = 0
            while True:
                if self.stop_event is not None and self.stop_event.is_set():
                    raise PpmError("cancelled")
                if reader is not None:
                    w, h = hd.width, hd.height
                    fdtype = np.uint16 if self.color.out_bits == 16 else np.uint8
                    nstage = hd.frame_bytes       # what crosses the pipe and PCIe; the budget counts the RGB frame, as for PPM
                else:
                    head = read_ppm_header(out)
                    if head is None:
                        break
                    w, h, maxval = head
                    if maxval not in (255, 65535):
                        raise PpmError("decoder delivered {}-level samples; the engine takes 8- or 16-bit frames".format(maxval + 1))
                    fdtype = np.uint16 if maxval == 65535 else np.uint8
                nbytes = w * h * 3 * np.dtype(fdtype).itemsize
                if reader is None:
                    nstage = nbytes
                st = self.state_for(k)
                # two pinned staging blocks per device: the pipe read of frame k overlaps the H2D copy of frame k-1
                pair = pinned.get((id(st), nstage))
                if pair is None:
                    pair = pinned[(id(st), nstage)] = [st.ctx.pinned(nstage), st.ctx.pinned(nstage)]
                which = turn.get(id(st), 0)        # the device's two staging blocks in turn
                stage = pair[which]
                host = np.frombuffer(stage.view, dtype=np.uint8, count=nstage)      # the pinned block as an array
                if reader is None:
                    read_exact_into(out, memoryview(host))
                elif not reader.read_into(host):
                    break
                turn[id(st)] = which ^ 1
                if pending is not None:           # frame k-1 has had this whole pipe read to land
                    pst, pev, pargs = pending
                    pst.ctx.event_sync(pst.upload_slot, pev)
                    self._publish(*pargs)
                    pending = None
                with self.cond:
                    self._make_room(nbytes)
                if reader is not None and (id(st), nstage) not in blocks:
                    # two device plane blocks per device, outside the budget like the pinned blocks.  Stream order alone makes their
                    # reuse safe: a block's previous conversion precedes the next upload into it on the same (upload) stream.
                    mine = blocks[(id(st), nstage)] = (st, [])
                    for _ in range(2):
                        mine[1].append(self._alloc(st, nstage))
                buf = self._alloc(st, nbytes)
                ev = _EVENT_BASE + which
                try:
                    with st.upload_lock:          # the engine's still-image uploads share this stream (engine.resident_frame)
                        if reader is not None:
                            block = blocks[(id(st), nstage)][1][which]
                            st.ctx.upload(block, host, slot=st.upload_slot, sync=False)
                            n_y, n_c = (ph * pw * hd.dtype.itemsize for ph, pw in hd.plane_shapes[:2])
                            self.color.convert_dev(st.ctx, [(block.ptr, block.ptr + n_y, block.ptr + n_y + n_c, w, h, hd.subsampling, buf)],
                                                   slot=st.upload_slot)
                        else:
                            st.ctx.upload(buf, host, slot=st.upload_slot, sync=False)
                            if fdtype == np.uint16:           # PPM samples are big-endian: swapped on the device, behind the copy
                                st.ctx.bswap16(buf, nbytes // 2, slot=st.upload_slot)
                        st.ctx.event_record(st.upload_slot, ev)
                except Exception:
                    st.ctx.free(buf)              # not published, not pending: nobody else would release it
                    raise
                if reader is not None:
                    self.plane_fed_frames += 1
                    if self.feed_stats is not None:
                        self.feed_stats.add(1, 0)
                pending = (st, ev, (st, buf, h, w, fdtype, nbytes))
                k += 1
            if pending is not None:
                pst, pev, pargs = pending
                pst.ctx.event_sync(pst.upload_slot, pev)
                self._publish(*pargs)
                pending = None
            rc = self.proc.wait()
            if rc != 0:
                errlog.seek(max(0, errlog.seek(0, os.SEEK_END) - 2000))
                text = errlog.read().decode(errors="ignore").strip()
                raise PpmError("decoder exited with code {}: {}".format(rc, text[-400:]))
        except Exception as exc:  # noqa: BLE001  (reported to every waiting view job)
            with self.cond:
                self.error = str(exc)
            if self.proc is not None and self.proc.poll() is None:
                try:
                    self.proc.kill()
                except Exception:
                    pass
            if pending is not None:               # the copy may still be running: let it finish before its blocks are freed
                try:
                    pending[0].ctx.event_sync(pending[0].upload_slot, pending[1])
                    if pending[0].ctx.handle:
                        pending[0].ctx.free(pending[2][1])
                except Exception:
                    pass
        finally:
            for pair in pinned.values():
                for stage in pair:
                    stage.free()
            for bst, pair in blocks.values():     # (freeing device memory waits for the stream's work on it)
                for block in pair:
                    try:
                        if bst.ctx.handle:
                            bst.ctx.free(block)
                    except Exception:
                        pass
            if errlog is not None:
                errlog.close()
            if self.proc is not None and self.register_proc:
                self.register_proc(self.proc, False)
            with self.cond:
                self.finished = True
                self.cond.notify_all()

    # view jobs -------------------------------------------------------------------------------------------------
    def join(self):
        """Register a view job -> token, or None when the video's first frames have already been retired (a job can only
        walk the video from its beginning)."""
        with self.cond:
            if self.first > 0:
                return None
            tok = self._next_token
            self._next_token += 1
            self.cursors[tok] = 0
            self.active_jobs += 1
            return tok

    def leave(self, token):
        with self.cond:
            if self.cursors.pop(token, None) is not None:
                self.active_jobs -= 1
                self.done_jobs += 1
            self.cond.notify_all()

    def state_for(self, k: int):
        """the device frame k is (or will be) resident on: blocks of _WINDOW frames round-robin"""
        return self.states[(k // _WINDOW) % len(self.states)]

    def advance(self, token, k: int):
        """the job `token` declares frames < k done (without asking for one)"""
        with self.cond:
            if token in self.cursors and k > self.cursors[token]:
                self.cursors[token] = k
                self.cond.notify_all()

    def window(self, token, k0: int, limit: int = _WINDOW):
        """frames k0, k0 + 1, ... of ONE device for one batched launch: waits for frame k0 like frame(), then takes its successors -- at
        most `limit`, never past the end of k0's block -- as (state, [DeviceBuffer], H, W, dtype); None after the last frame.  For the
        rest of the window it waits only while the decoder is still delivering, and at most _WINDOW_WAIT_S in all: the reader may be
        blocked at its budget until this very job moves on (a bounded wait cannot deadlock; a decoder slower than that is the
        bottleneck whatever the window)."""
        first = self.frame(token, k0)
        if first is None:
            return None
        st, buf, h, w, dt = first
        end = min(k0 + max(1, limit), (k0 // _WINDOW + 1) * _WINDOW)
        bufs = [buf]
        deadline = time.monotonic() + _WINDOW_WAIT_S
        with self.cond:
            while self.count < end and not self.finished and not self.closing:
                left = deadline - time.monotonic()
                if left <= 0 or (self.stop_event is not None and self.stop_event.is_set()):
                    break
                self.cond.wait(timeout=left)
            for k in range(k0 + 1, min(end, self.count)):
                fr = self.frames.get(k)
                if fr is None or fr[0] is not st or fr[2:] != (h, w, dt):
                    break
                bufs.append(fr[1])
        return st, bufs, h, w, dt

    def frame(self, token, k: int):
        """k-th decoded frame as (state, DeviceBuffer, H, W, dtype) for the job `token`, which thereby declares frames < k
        done; None after the last one.  Raises on decoder failure."""
        with self.cond:
            if token in self.cursors and k > self.cursors[token]:
                self.cursors[token] = k
                self.cond.notify_all()            # the reader may be waiting for exactly this
            while k >= self.count and not self.finished:
                self.cond.wait(timeout=0.25)
                if self.stop_event is not None and self.stop_event.is_set():
                    return None
            if k < self.count:
                if k < self.first:
                    raise PpmError("frame {} was retired before this view job asked for it".format(k))
                return self.frames[k]
            if self.error:
                raise PpmError(self.error)
            return None

    def close(self):
        if self.proc is not None and self.proc.poll() is None:
            try:
                self.proc.kill()
            except Exception:
                pass
        with self.cond:
            self.closing = True
            self.cursors.clear()
            self.cond.notify_all()
        self.thread.join(timeout=5.0)
        if self.color is not None and not self.thread.is_alive():
            self.color.close()
            self.color = None
        with self.cond:
            for st, buf, _h, _w, _dt in self.frames.values():
                if st.ctx.handle:
                    st.ctx.free(buf)
            self.frames = {}
            self.shared.add(-self.bytes)
            self.bytes = 0
