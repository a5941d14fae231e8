"""Incremental reader of a YUV4MPEG2 stream from a pipe: the header's geometry, then the three planes of every FRAME.

The stream carries its own size, subsampling, depth and range (as the PPM pipe of gs360/video.py carries its size), so the decoder
that writes it needs no separate probe.  What gs360/vidcolor.py cannot convert is one Y4MError: a monochrome stream, 12 bits and
above, interlaced material, a truncated frame.
"""
import dataclasses

import numpy as np

# C tag -> (subsampling, depth); the 4:2:0 variants differ in chroma siting only, which VID-COLOR v1 (replicated chroma) ignores
COLORSPACES = {"420jpeg": ("420", 8), "420mpeg2": ("420", 8), "420paldv": ("420", 8), "420": ("420", 8), "422": ("422", 8),
               "444": ("444", 8), "420p10": ("420", 10), "422p10": ("422", 10), "444p10": ("444", 10)}
MAX_HEADER = 4096


class Y4MError(ValueError):
    pass


@dataclasses.dataclass(frozen=True)
class Y4MHeader:
    width: int
    height: int
    subsampling: str          # "420", "422" or "444"
    depth: int                # 8 or 10
    full_range: bool
    colorspace: str           # the C tag as written

    @property
    def dtype(self):
        return np.dtype(np.uint8 if self.depth == 8 else "<u2")

    @property
    def chroma_shape(self):
        sx, sy = {"444": (0, 0), "422": (1, 0), "420": (1, 1)}[self.subsampling]
        return (self.height + sy) >> sy, (self.width + sx) >> sx

    @property
    def plane_shapes(self):
        return (self.height, self.width), self.chroma_shape, self.chroma_shape

    @property
    def frame_bytes(self):
        return sum(h * w for h, w in self.plane_shapes) * self.dtype.itemsize


def _read_line(stream, what):
    """up to and without the next newline; b"" at a clean end of the stream"""
    line = bytearray()
    while True:
        c = stream.read(1)
        if not c:
            if line:
                raise Y4MError("Y4M stream ends inside {}".format(what))
            return b""
        if c == b"\n":
            return bytes(line)
        line += c
        if len(line) > MAX_HEADER:
            raise Y4MError("Y4M {} longer than {} bytes".format(what, MAX_HEADER))


def _read_exact(stream, view):
    """fill the writable buffer `view` from the stream; the bytes read (short at the end of the stream)"""
    got = 0
    while got < len(view):
        n = stream.readinto(view[got:])
        if not n:
            break
        got += n
    return got


def parse_header(line: bytes) -> Y4MHeader:
    fields = line.decode("ascii", errors="replace").split(" ")
    if fields[0] != "YUV4MPEG2":
        raise Y4MError("not a YUV4MPEG2 stream (starts with {!r})".format(line[:16]))
    width = height = 0
    tag, interlace, full = "420jpeg", "p", False
    for f in fields[1:]:
        if not f:
            continue
        key, val = f[0], f[1:]
        try:
            if key == "W":
                width = int(val)
            elif key == "H":
                height = int(val)
        except ValueError:
            raise Y4MError("bad Y4M header field {!r}".format(f)) from None
        if key == "C":
            tag = val
        elif key == "I":
            interlace = val
        elif f.startswith("XCOLORRANGE="):
            rng = f.split("=", 1)[1].upper()
            if rng not in ("FULL", "LIMITED"):
                raise Y4MError("unknown Y4M colour range {!r}".format(rng))
            full = rng == "FULL"
    if width < 1 or height < 1:
        raise Y4MError("Y4M header without a size (W{} H{})".format(width, height))
    if interlace in ("t", "b", "m"):
        raise Y4MError("interlaced Y4M stream (I{}): only progressive frames are converted".format(interlace))
    if tag not in COLORSPACES:
        raise Y4MError("unsupported Y4M colourspace C{}: 8- and 10-bit 4:2:0, 4:2:2 and 4:4:4 are converted".format(tag))
    sub, depth = COLORSPACES[tag]
    return Y4MHeader(width, height, sub, depth, full, tag)


class Y4MReader:
    """reader = Y4MReader(pipe); reader.header; for planes in reader: ...   (planes = (y, cb, cr) arrays)

    read_into(buffer) fills a caller's buffer of header.frame_bytes (pinned staging memory) instead of allocating."""

    def __init__(self, stream):
        self.stream = stream
        line = _read_line(stream, "the stream header")
        if not line:
            raise Y4MError("empty Y4M stream")
        self.header = parse_header(line)
        self.frames_read = 0

    def read_into(self, buffer) -> bool:
        """the next frame's bytes (Y, Cb, Cr back to back) into `buffer`; False at the end of the stream"""
        line = _read_line(self.stream, "a frame header")
        if not line:
            return False
        if not line.startswith(b"FRAME"):
            raise Y4MError("expected FRAME, found {!r}".format(line[:16]))
        need = self.header.frame_bytes
        view = memoryview(buffer).cast("B")[:need]
        got = _read_exact(self.stream, view)
        if got != need:
            raise Y4MError("truncated Y4M frame {}: {} of {} bytes".format(self.frames_read, got, need))
        self.frames_read += 1
        return True

    def split(self, buffer):
        """the three planes of a frame held in `buffer` (views, not copies)"""
        h = self.header
        flat = np.frombuffer(buffer, dtype=np.uint8, count=h.frame_bytes)
        planes, at = [], 0
        for ph, pw in h.plane_shapes:
            n = ph * pw * h.dtype.itemsize
            planes.append(flat[at:at + n].view(h.dtype).reshape(ph, pw))
            at += n
        return tuple(planes)

    def __iter__(self):
        while True:
            buf = bytearray(self.header.frame_bytes)
            if not self.read_into(buf):
                return
            yield self.split(buf)
