"""The FrameSelector's reader under GS360_JPEG_DECODER=device: paths -> frames for the scoring, edge and flow passes.

A file named .jpg / .jpeg that jpegdec.parse() accepts and that the device decodes with status 0 becomes a
framescore.DeviceFrame(buf, H, W, 1, stride): the gray plane of gs360_jpeg_decode_gray_u8, which is all the three passes read of a
pixel (gray_of<C>, csrc/gs360_framepx.h), bit for bit what they compute from the RGB frame.  Every other file (not a JPEG by name,
refused by parse(), a non-zero device status, a Gs360Error from the decode call) goes through the pass's own host decode and gives
today's ndarray or None.  Results keep the order of the paths.

The pool threads do the host-only part (Reader.load: the file read, parse, the segment table, the scratch size); the consuming
thread queues the decode batches (Reader.resolve: up to GS360_MAX_FRAMES files per call, on the context's slot 0 under its lock) and
then the pass's own launch.

open_store() keeps the planes decoded for scoring resident for the flow pass, keyed by absolute path, first come until the budget
(GS360_FS_GRAY_CACHE_MB, 16384) is reached: both passes walk the records from the front, so evicting the least recently used frame
would discard exactly what the flow pass asks for first.  Without an open store nothing outlives the Reader that decoded it.

With GS360_JPEG_DECODER=host (the default) nothing here runs: framescore and frameflow ask jpegdec.device_decoder_enabled() first.
"""
import collections
import contextlib
import logging
import os
import threading

from . import capi, framescore, jpegdec

log = logging.getLogger("gs360.framesource")

DEFAULT_CACHE_MB = 16384

_lock = threading.Lock()
_store = None
_files = {"device_decoded": set(), "fallbacks": set()}     # the distinct files of each kind: a file both passes read counts once
_reused = [0]


def stats():
    """-> {device_decoded: files decoded on the device, fallbacks: files the host decoded, reused: frames a pass took from the store
    instead of the file, kept_bytes: what the open store holds} of this process since reset_stats()"""
    with _lock:
        out = {k: len(v) for k, v in _files.items()}
        out["reused"] = _reused[0]
        out["kept_bytes"] = _store.kept_bytes if _store is not None else 0
    return out


def reset_stats():
    with _lock:
        for v in _files.values():
            v.clear()
        _reused[0] = 0


def _count(name, path):
    with _lock:
        if name == "reused":
            _reused[0] += 1
        else:
            _files[name].add(os.path.abspath(path))


def default_budget():
    """GS360_FS_GRAY_CACHE_MB in bytes"""
    text = os.environ.get("GS360_FS_GRAY_CACHE_MB", str(DEFAULT_CACHE_MB))
    try:
        mb = int(text)
    except ValueError:
        raise ValueError(f"GS360_FS_GRAY_CACHE_MB must be a whole number of MiB (got {text!r})") from None
    return max(0, mb) << 20


class Store:
    """Gray planes that stay in device memory between the passes of one run: path -> DeviceFrame, first come until the budget."""

    def __init__(self, budget_bytes):
        self.budget = int(budget_bytes)
        self.frames = {}                 # absolute path -> (ctx, DeviceFrame)
        self.kept_bytes = 0
        self.keeping = True

    def get(self, path):
        with _lock:
            hit = self.frames.get(os.path.abspath(path))
        return hit[1] if hit else None

    def offer(self, ctx, path, frame):
        """-> True when the store now owns the frame's buffer"""
        nbytes = frame.H * (frame.stride or frame.W * frame.C)
        key = os.path.abspath(path)
        with _lock:
            if not self.keeping or key in self.frames:
                return False
            if self.kept_bytes + nbytes > self.budget:
                self.keeping = False     # first come: what follows is not kept either
                return False
            self.frames[key] = (ctx, frame)
            self.kept_bytes += nbytes
        return True

    def stop_keeping(self):
        with _lock:
            self.keeping = False

    def close(self):
        with _lock:
            frames, self.frames = self.frames, {}
            self.kept_bytes = 0
            self.keeping = False
        for ctx, frame in frames.values():
            ctx.free(frame.buf)


@contextlib.contextmanager
def open_store(budget_bytes=None):
    """While open, the gray planes a Reader(keep=True) decodes stay resident (up to budget_bytes; None = GS360_FS_GRAY_CACHE_MB) and
    later Readers take them from here.  Everything is freed on exit, whatever ends the block."""
    global _store
    reset_stats()
    store = Store(default_budget() if budget_bytes is None else budget_bytes)
    with _lock:
        if _store is not None:
            raise RuntimeError("a frame store is already open")
        _store = store
    try:
        yield store
    finally:
        with _lock:
            _store = None
        store.close()


def current_store():
    with _lock:
        return _store


def device_decode(ctx, prepared):
    """prepared: jpegdec.Prepared of up to GS360_MAX_FRAMES files -> [DeviceFrame (the gray plane) or None], one decode call on slot 0.
    A Gs360Error (out of device memory, say) gives None for every file and ends the store's keeping."""
    try:
        results = jpegdec.decode_device(ctx, prepared, slot=0, gray=True)
    except capi.Gs360Error as exc:
        log.debug("host JPEG decode for %d files (%s)", len(prepared), exc)
        store = current_store()
        if store is not None:
            store.stop_keeping()
        return [None] * len(prepared)
    out = []
    for r in results:
        if r.buf is None:
            log.debug("host JPEG decode (%s)", r.reason)
            out.append(None)
        else:
            out.append(framescore.DeviceFrame(r.buf, r.shape[0], r.shape[1], 1, r.stride))
    return out


class _Host:
    """what the pass's host decode gave for a file the device path does not take"""
    __slots__ = ("frame",)

    def __init__(self, frame):
        self.frame = frame


class Reader:
    """One pass's reader.  decode: the pass's host decode, path -> ndarray or None (called for the fallback files only, once each);
    keep: offer what is decoded to the open store.  A context manager: on exit every device frame it handed out that the store does
    not own is freed (release() frees earlier)."""

    def __init__(self, ctx, decode, keep=False):
        self.ctx, self.decode, self.keep = ctx, decode, keep
        self.owned = {}                  # id(buf) -> buf

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        owned, self.owned = self.owned, {}
        for buf in owned.values():
            self.ctx.free(buf)
        return False

    def load(self, path):
        """The host-only part, for a pool thread: -> a DeviceFrame of the store, a jpegdec.Prepared, or the host decode's result"""
        if not jpegdec.is_jpeg_path(path):
            return _Host(self.decode(path))
        store = current_store()
        hit = store.get(path) if store is not None else None
        if hit is not None:
            return hit
        try:
            with open(path, "rb") as f:
                data = f.read()
            return jpegdec.prepare(data)
        except (OSError, jpegdec.Unsupported) as exc:
            log.debug("%s: host JPEG decode (%s)", path, exc)
            return _Host(self.decode(path))           # (an unreadable file: the host reader reports it its own way)

    def resolve(self, paths, loaded):
        """loaded: load()'s results for paths -> the frames in that order (DeviceFrame, ndarray or None); queues the decode calls"""
        out = [None] * len(paths)
        todo = []
        for i, item in enumerate(loaded):
            if isinstance(item, jpegdec.Prepared):
                todo.append(i)
            elif isinstance(item, _Host):
                out[i] = item.frame
                _count("fallbacks", paths[i])
            else:
                out[i] = item
                _count("reused", paths[i])
        store = current_store() if self.keep else None
        for c in range(0, len(todo), capi.MAX_FRAMES):
            part = todo[c:c + capi.MAX_FRAMES]
            for i, fr in zip(part, device_decode(self.ctx, [loaded[i] for i in part])):
                if fr is None:
                    out[i] = self.decode(paths[i])
                    _count("fallbacks", paths[i])
                    continue
                out[i] = fr
                _count("device_decoded", paths[i])
                if store is None or not store.offer(self.ctx, paths[i], fr):
                    self.owned[id(fr.buf)] = fr.buf
        return out

    def read(self, paths):
        """-> the frames of paths, in order, without a pool"""
        return self.resolve(paths, [self.load(p) for p in paths])

    def release(self, frames):
        """frees the device frames among `frames` that this reader owns (the store's stay)"""
        for fr in frames:
            if isinstance(fr, framescore.DeviceFrame):
                buf = self.owned.pop(id(fr.buf), None)
                if buf is not None:
                    self.ctx.free(buf)

    def frames(self, paths, ex, window):
        """(index, frame) for every path, in order: load() runs on the pool `ex`, at most `window` files ahead"""
        futs = collections.deque()
        nxt = 0
        while nxt < len(paths) or futs:
            while nxt < len(paths) and len(futs) < window:
                futs.append((nxt, ex.submit(self.load, paths[nxt])))
                nxt += 1
            head = [futs.popleft() for _ in range(min(len(futs), capi.MAX_FRAMES))]
            loaded = [f.result() for _, f in head]
            for (k, _), fr in zip(head, self.resolve([paths[k] for k, _ in head], loaded)):
                yield k, fr
