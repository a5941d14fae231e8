"""Baseline JPEG files decoded on the device (JPD-SPEC v1).

parse() walks a file's marker segments on the host and returns what the device needs: the geometry, the quantiser and Huffman tables
and where the entropy-coded segment and its restart intervals lie.  decode_device() uploads only those bytes; gs360_jpeg_decode_u8
(csrc/gs360_jpegdec.hip) decodes the scan with the self-synchronising parallel Huffman scheme, rebuilds the pixels with libjpeg's
integer arithmetic (islow IDCT, the upsampling of the file's chroma layout, the fixed-point YCbCr -> RGB rows) and leaves an H x W x C uint8 image in
device memory, byte for byte what Pillow / libjpeg-turbo return for the file.  Whatever parse() refuses (Unsupported) the host decodes.
With gray=True the call is gs360_jpeg_decode_gray_u8 and the result an H x W plane of FS-SPEC's gray of those pixels, which is all the
FrameSelector's passes read (gs360/framesource.py).  prepare() is the part of a decode that needs neither a device nor a lock.

Restart markers are found on the host, with vectorised NumPy: the scan's bytes are in host memory anyway before their upload, one
comparison pass over them costs less than their PCIe copy, and the device then gets every segment's start, length and first
subsequence as a table instead of searching for markers itself.
"""
import ctypes as ct
import logging
import os

import numpy as np

from . import capi

log = logging.getLogger("gs360.jpegdec")

TABLE_BYTES = capi.JPEG_TABLE_BYTES
MAX_BYTES = (1 << 31) - 1            # 32-bit offsets on the device: larger files go to the host


class Unsupported(ValueError):
    """the file is not one the device path takes (the host decodes it)"""


# component sampling bytes (Y, Cb, Cr) -> `subsampling`: what parse() takes by default, and everything the device decodes
V1_SAMPLINGS = {(0x11, 0x11, 0x11): capi.JPEG_444, (0x22, 0x11, 0x11): capi.JPEG_420}
DEVICE_SAMPLINGS = dict(V1_SAMPLINGS)
DEVICE_SAMPLINGS.update({(0x21, 0x11, 0x11): capi.JPEG_422, (0x12, 0x11, 0x11): capi.JPEG_440, (0x41, 0x11, 0x11): capi.JPEG_411})
# `subsampling` -> the luma sampling (horizontal, vertical) over 1 x 1 chroma
LUMA_SAMPLING = {capi.JPEG_444: (1, 1), capi.JPEG_422: (2, 1), capi.JPEG_420: (2, 2), capi.JPEG_440: (1, 2), capi.JPEG_411: (4, 1)}


class Descriptor:
    """What parse() found.  H, W, C; subsampling (capi.JPEG_444 / JPEG_422 / JPEG_420 / JPEG_440 / JPEG_411; JPEG_444 for gray); restart (MCUs per restart interval, 0 =
    none); quant: uint8 [4][64] in file (zig-zag) order; huff: uint8 [4][272] (DC0, AC0, DC1, AC1: 16 BITS + HUFFVAL, zero padded);
    comp_tq / comp_td / comp_ta: per component the quantiser, DC and AC table it uses; scan_off, scan_len: the entropy-coded segment
    in the file (everything between the SOS header and EOI); segments: uint32 [n][2], start (relative to scan_off) and length of every
    restart interval's bytes, RSTn markers excluded."""
    __slots__ = ("H", "W", "C", "subsampling", "restart", "quant", "huff", "comp_tq", "comp_td", "comp_ta", "scan_off", "scan_len",
                 "segments")

    @property
    def luma_sampling(self):
        """(hs, vs): an MCU holds hs x vs Y blocks in raster order, then (C = 3) Cb and Cr"""
        return LUMA_SAMPLING[self.subsampling] if self.C == 3 else (1, 1)

    @property
    def mcu_px(self):
        """(height, width) of an MCU in pixels"""
        hs, vs = self.luma_sampling
        return 8 * vs, 8 * hs

    mcu_h = property(lambda self: self.mcu_px[0])
    mcu_w = property(lambda self: self.mcu_px[1])

    @property
    def blocks_per_mcu(self):
        hs, vs = self.luma_sampling
        return hs * vs + 2 if hs * vs > 1 else self.C

    @property
    def mcu_grid(self):
        ph, pw = self.mcu_px
        return (self.H + ph - 1) // ph, (self.W + pw - 1) // pw

    @property
    def n_mcu(self):
        mh, mw = self.mcu_grid
        return mh * mw


def _u16(data, at):
    return (data[at] << 8) | data[at + 1]


def find_segments(scan, restart, n_mcu):
    """scan: uint8 array of the entropy-coded segment -> uint32 [n][2] (start, length) of the restart intervals.  Vectorised: a marker
    is 0xFF followed by anything but 0x00 (a stuffed byte) or 0xFF (fill)."""
    ff = np.flatnonzero(scan[:-1] == 0xFF) if scan.size > 1 else np.zeros(0, np.int64)
    nxt = scan[ff + 1]
    marks = ff[(nxt != 0x00) & (nxt != 0xFF)]
    codes = scan[marks + 1]
    want = (n_mcu + restart - 1) // restart - 1 if restart else 0
    if marks.size != want or np.any(codes != (0xD0 + (np.arange(marks.size) & 7))):
        raise Unsupported("the scan's restart markers do not match its restart interval")
    if np.any(scan[ff + 1] == 0xFF):
        raise Unsupported("fill bytes inside the scan")
    starts = np.concatenate(([0], marks + 2))
    ends = np.concatenate((marks, [scan.size]))
    return np.stack([starts, ends - starts], axis=1).astype(np.uint32)


def parse(data, samplings=V1_SAMPLINGS):
    """data: the bytes of a file -> Descriptor, or raises Unsupported(reason).  samplings: the component layouts of a colour file to
    accept, {(Y, Cb, Cr sampling bytes): subsampling}; the default is gray, 4:4:4 and 4:2:0 only, DEVICE_SAMPLINGS all the device takes"""
    data = bytes(data)
    n = len(data)
    if n > MAX_BYTES:
        raise Unsupported("file of 2^31 bytes or more")
    if n < 4 or data[:2] != b"\xff\xd8":
        raise Unsupported("not a JPEG file")
    d = Descriptor()
    d.quant = np.zeros((4, 64), np.uint8)
    d.huff = np.zeros((4, TABLE_BYTES), np.uint8)
    d.restart = 0
    have_q, have_h = set(), set()
    sof = None
    adobe_transform = None
    at = 2
    while True:
        if at + 4 > n:
            raise Unsupported("the file ends inside its header")
        if data[at] != 0xFF:
            raise Unsupported("no marker where one is due")
        m = data[at + 1]
        if m == 0xFF:                    # fill byte
            at += 1
            continue
        if m == 0xD8 or 0xD0 <= m <= 0xD7 or m == 0x01:
            at += 2
            continue
        if m == 0xD9:
            raise Unsupported("EOI before a scan")
        seg_len = _u16(data, at + 2)
        if seg_len < 2 or at + 2 + seg_len > n:
            raise Unsupported("the file ends inside a segment")
        body = data[at + 4:at + 2 + seg_len]
        if m == 0xC0:
            if sof is not None:
                raise Unsupported("two frame headers")
            if len(body) < 6 or len(body) != 6 + 3 * body[5]:
                raise Unsupported("malformed SOF0")
            if body[0] != 8:
                raise Unsupported(f"{body[0]}-bit samples")
            sof = (_u16(body, 1), _u16(body, 3), [(body[6 + 3 * k], body[7 + 3 * k], body[8 + 3 * k]) for k in range(body[5])])
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            raise Unsupported("not baseline sequential Huffman coding (SOF%d)" % (m - 0xC0))
        elif m == 0xCC:
            raise Unsupported("arithmetic coding")
        elif m == 0xDB:
            k = 0
            while k < len(body):
                pq, tq = body[k] >> 4, body[k] & 15
                if pq != 0:
                    raise Unsupported("16-bit quantiser table")
                if tq > 3 or k + 65 > len(body):
                    raise Unsupported("malformed DQT")
                d.quant[tq] = np.frombuffer(body, np.uint8, 64, k + 1)
                have_q.add(tq)
                k += 65
        elif m == 0xC4:
            k = 0
            while k < len(body):
                if k + 17 > len(body):
                    raise Unsupported("malformed DHT")
                tc, th = body[k] >> 4, body[k] & 15
                count = sum(body[k + 1:k + 17])
                if tc > 1 or th > 1 or count > 256 or k + 17 + count > len(body):
                    raise Unsupported("Huffman table outside baseline (class %d, id %d)" % (tc, th))
                # every code must fit its length (a table that over-subscribes the code space is refused, as libjpeg does)
                code = 0
                for ln in range(16):
                    code = (code + body[k + 1 + ln]) << 1
                    if code > (2 << (ln + 1)):
                        raise Unsupported("Huffman table over-subscribes its code space")
                slot = th * 2 + tc
                d.huff[slot] = 0
                d.huff[slot, :16 + count] = np.frombuffer(body, np.uint8, 16 + count, k + 1)
                have_h.add(slot)
                k += 17 + count
        elif m == 0xDD:
            if len(body) != 2:
                raise Unsupported("malformed DRI")
            d.restart = _u16(body, 0)
        elif m == 0xEE and body[:5] == b"Adobe" and len(body) >= 12:
            adobe_transform = body[11]
        elif m == 0xDA:
            break
        # APPn, COM and anything else with a length: skipped
        at += 2 + seg_len
    if sof is None:
        raise Unsupported("a scan before the frame header")
    H, W, comps = sof
    if H < 1 or W < 1:
        raise Unsupported("empty image (or DNL-defined height)")
    if len(comps) not in (1, 3):
        raise Unsupported(f"{len(comps)} components")
    sampling = tuple(c[1] for c in comps)
    if len(comps) == 1:
        d.subsampling = capi.JPEG_444        # a single component's sampling factors do not matter: its MCU is one block
    elif sampling in samplings:
        d.subsampling = samplings[sampling]
    else:
        raise Unsupported("sampling factors " + ",".join("%02x" % s for s in sampling))
    if len(comps) == 3 and adobe_transform is not None and adobe_transform != 1:
        raise Unsupported("Adobe colour transform %d" % adobe_transform)
    if len(comps) == 3 and adobe_transform is None and [c[0] for c in comps] == [0x52, 0x47, 0x42]:
        raise Unsupported("components marked R, G, B")      # libjpeg reads these ids as RGB, not YCbCr
    sos = body
    if len(sos) < 1 or len(sos) != 4 + 2 * sos[0]:
        raise Unsupported("malformed SOS")
    if sos[0] != len(comps):
        raise Unsupported("a scan that does not hold every component (multiple scans)")
    d.comp_tq, d.comp_td, d.comp_ta = [], [], []
    for k, (cid, _s, tq) in enumerate(comps):
        if sos[1 + 2 * k] != cid:
            raise Unsupported("scan components out of frame order")
        td, ta = sos[2 + 2 * k] >> 4, sos[2 + 2 * k] & 15
        if td > 1 or ta > 1 or td * 2 not in have_h or ta * 2 + 1 not in have_h or tq not in have_q:
            raise Unsupported("a component uses a table the file does not define")
        d.comp_tq.append(tq)
        d.comp_td.append(td)
        d.comp_ta.append(ta)
    if tuple(sos[-3:]) != (0, 63, 0):
        raise Unsupported("spectral selection or successive approximation")
    d.H, d.W, d.C = H, W, len(comps)
    d.scan_off = at + 2 + seg_len
    # the scan runs to EOI, which must be the file's next marker segment after it
    raw = np.frombuffer(data, np.uint8)
    end = data.rfind(b"\xff\xd9")
    if end < d.scan_off:
        raise Unsupported("no EOI: the file is cut short")
    d.scan_len = end - d.scan_off
    if d.scan_len < 1:
        raise Unsupported("empty scan")
    d.segments = find_segments(raw[d.scan_off:end], d.restart, d.n_mcu)      # (any other marker inside, a second SOS included, is refused there)
    return d


# ---- the device call --------------------------------------------------------------------------------------------------------------
def subseq_bytes():
    """bytes of the compressed stream one lane decodes first (GS360_JPEG_DEC_SUBSEQ_BYTES)"""
    return capi.JPEG_DEC_SUBSEQ_BYTES


def subseqs_per_workgroup():
    """subsequences one workgroup of the entropy stage synchronises among themselves (GS360_JPEG_DEC_WG_SUBSEQS)"""
    return capi.JPEG_DEC_WG_SUBSEQS


def segment_table(d):
    """uint32 [n][4] for the device: start, length, first subsequence, first MCU of every restart interval"""
    seg = d.segments.astype(np.int64)
    subs = (seg[:, 1] + capi.JPEG_DEC_SUBSEQ_BYTES - 1) // capi.JPEG_DEC_SUBSEQ_BYTES
    first = np.concatenate(([0], np.cumsum(subs)[:-1]))
    mcu0 = np.arange(seg.shape[0], dtype=np.int64) * (d.restart if d.restart else 0)
    return np.stack([seg[:, 0], seg[:, 1], first, mcu0], axis=1).astype(np.uint32), int(subs.sum())


def scratch_bytes(d, n_subseq=None):
    """gs360_jpeg_decode_scratch: the scratch one job needs"""
    if n_subseq is None:
        n_subseq = segment_table(d)[1]
    n = ct.c_size_t(0)
    L = capi.load_library()
    capi._check(L.gs360_jpeg_decode_scratch(d.H, d.W, d.C, d.subsampling, int(n_subseq), ct.byref(n)), L)
    return int(n.value)


class Decoded:
    """One decode_device result: buf (DeviceBuffer holding H rows of `stride` bytes, or None where the file went to the host), shape
    (H, W, C), stride, status (0 = decoded on the device; the device's reason code; -1 = parse() refused the file) and `reason`."""
    __slots__ = ("buf", "shape", "stride", "status", "reason")

    def __init__(self, buf, shape, stride, status, reason=""):
        self.buf, self.shape, self.stride, self.status, self.reason = buf, shape, stride, status, reason


class Prepared:
    """The host-only part of one file's decode: its bytes, parse()'s Descriptor, the segment table, the subsequence count and the
    scratch the device needs.  prepare() makes it without touching a device or a lock, so that a pool thread can; Batch takes it in
    place of the file's bytes."""
    __slots__ = ("data", "d", "seg", "n_sub", "nscr")

    def __init__(self, data, d, seg, n_sub, nscr):
        self.data, self.d, self.seg, self.n_sub, self.nscr = data, d, seg, n_sub, nscr


def prepare(data):
    """data: the bytes of a file -> Prepared, or raises Unsupported(reason) as parse() does"""
    d = parse(data, samplings=DEVICE_SAMPLINGS)
    seg, n_sub = segment_table(d)
    return Prepared(data, d, seg, n_sub, scratch_bytes(d, n_sub))


class Batch:
    """The device side of one decode call: per accepted file its scan, segment table and tables uploaded, scratch and output
    allocated.  datas: per file its bytes, or what prepare() made of them (then only allocations and uploads happen here).  gray: the
    outputs are H x (W + pad) planes and run() queues gs360_jpeg_decode_gray_u8.  run() queues gs360_jpeg_decode_u8 (as often as
    wanted: the bench times it); close() frees everything but the outputs handed out."""

    def __init__(self, ctx, datas, slot=0, pad=0, guard=0, gray=False):
        self.ctx, self.slot, self.gray = ctx, slot, bool(gray)
        self.refused = {}                # index in datas -> reason
        self.items = []                  # (index in datas, Descriptor, out buffer, scratch buffer, scratch bytes, stride)
        self.jobs, self.owned = [], []
        self.uploaded = 0                # bytes sent to the device
        try:
            self._prepare(datas, pad, guard)
        except BaseException:
            self.close()                 # (an allocation or upload failed half way: nothing stays behind)
            raise

    def _prepare(self, datas, pad, guard):
        ctx, slot = self.ctx, self.slot
        sources = []
        for k, data in enumerate(datas):
            try:
                p = data if isinstance(data, Prepared) else prepare(data)
            except Unsupported as exc:
                self.refused[k] = str(exc)
                continue
            d, seg, n_sub, nscr = p.d, p.seg, p.n_sub, p.nscr
            scan = np.frombuffer(p.data, np.uint8, d.scan_len, d.scan_off)
            meta = np.concatenate([d.huff.reshape(-1), d.quant.reshape(-1)])
            stride = d.W * (1 if self.gray else d.C) + int(pad)
            b_scan, b_seg, b_meta, b_scr, b_out = (self._alloc(n) for n in (scan.nbytes, seg.nbytes, meta.nbytes, nscr + guard, d.H * stride + guard))
            for b, a in ((b_scan, scan), (b_seg, seg), (b_meta, meta)):
                ctx.upload(b, a, slot, sync=False)
                sources.append(a)        # (alive until the sync below)
                self.uploaded += a.nbytes
            if pad or guard:
                ctx.memset(b_out, 0xA5, slot)
                ctx.memset(b_scr, 0xA5, slot)
            sel = [(ct.c_uint8 * 4)(*v) for v in (d.comp_tq, d.comp_td, d.comp_ta)]
            self.jobs.append(capi.JpegDecJob(b_scan.ptr, d.scan_len, n_sub, b_seg.ptr, seg.shape[0], b_meta.ptr, d.H, d.W, d.C, d.subsampling,
                                             d.restart, sel[0], sel[1], sel[2], b_scr.ptr, nscr, b_out.ptr, stride))
            self.items.append((k, d, b_out, b_scr, nscr, stride))
        self.d_status = self._alloc(4 * max(len(self.jobs), 1))
        ctx.sync(slot)                   # (the uploads' sources may go)

    def _alloc(self, nbytes):
        self.owned.append(self.ctx.alloc(nbytes))
        return self.owned[-1]

    def run(self):
        """queues the decode on the slot (asynchronous)"""
        if self.jobs:
            (self.ctx.jpeg_decode_gray_dev if self.gray else self.ctx.jpeg_decode_dev)(self.jobs, self.d_status, slot=self.slot)

    def status(self):
        """-> [status code per accepted file]; waits for the slot"""
        return [int(v) for v in self.ctx.download(self.d_status, (len(self.jobs),), np.uint32, self.slot)] if self.jobs else []

    def rounds(self):
        """-> per accepted file the rounds its entry states took to settle across workgroups (the scratch starts with three counters:
        invalid codes met, intervals that ended where they should, those rounds)"""
        return [int(self.ctx.download(b_scr, (4,), np.uint32, self.slot)[2]) for _k, _d, _o, b_scr, _n, _s in self.items]

    def release(self, buf):
        """the caller keeps `buf` (an output): close() leaves it alone"""
        self.owned = [b for b in self.owned if b is not buf]
        return buf

    def close(self):
        for b in self.owned:
            self.ctx.free(b)
        self.owned = []


def decode_device(ctx, datas, slot=0, gray=False):
    """datas: the bytes of JPEG files (or prepare()'s results) -> [Decoded], one gs360_jpeg_decode_u8 call on `slot` for all the files
    parse() accepts; gray: one gs360_jpeg_decode_gray_u8 call, the results are H x W planes of shape (H, W, 1).  Only
    the scans, the tables and the segment records are uploaded.  A file the device path did not take (parse() refused it, or the device
    reports a status != 0) has buf = None: the caller decodes it on the host.  The caller owns the buffers it gets."""
    results = [None] * len(datas)
    with ctx.slot_locks[slot]:
        batch = Batch(ctx, datas, slot, gray=gray)  # (frees what it allocated if it fails half way)
        try:
            for k, reason in batch.refused.items():
                results[k] = Decoded(None, None, 0, -1, reason)
            batch.run()
            for (k, d, b_out, _scr, _n, stride), code in zip(batch.items, batch.status()):
                buf = batch.release(b_out) if code == 0 else None
                results[k] = Decoded(buf, (d.H, d.W, 1 if gray else d.C), stride, code, "" if code == 0 else "device status %d" % code)
        finally:
            batch.close()
    return results


def decode_to_host(ctx, datas, slot=0):
    """-> ([ndarray H x W x C (H x W for gray) or None], [status]): decode_device and the downloads, for tests"""
    out, codes = [], []
    for r in decode_device(ctx, datas, slot):
        codes.append(r.status)
        if r.buf is None:
            out.append(None)
            continue
        H, W, C = r.shape
        a = ctx.download(r.buf, (H, W, C), np.uint8, slot)
        ctx.free(r.buf)
        out.append(a[:, :, 0] if C == 1 else a)
    return out, codes


def device_decoder_enabled():
    """GS360_JPEG_DECODER = host (default) | device"""
    mode = os.environ.get("GS360_JPEG_DECODER", "host")
    if mode not in ("host", "device"):
        raise ValueError(f"GS360_JPEG_DECODER must be host or device (got {mode!r})")
    return mode == "device"


def is_jpeg_path(path):
    return str(path).lower().endswith((".jpg", ".jpeg"))


def try_decode_file(ctx, path, slot=0):
    """-> Decoded with a device buffer, or None when the host has to decode the file (not a JPEG by name or content, refused by
    parse(), or a non-zero device status): the caller then goes on exactly as without the device decoder"""
    if not is_jpeg_path(path):
        return None
    try:
        with open(path, "rb") as f:
            data = f.read()
    except OSError:
        return None                      # the host reader reports it its own way
    try:
        r = decode_device(ctx, [data], slot)[0]
    except capi.Gs360Error as exc:
        # the device path needs the coefficients besides the frame, about twice the host path's device memory: when that (or anything
        # else in the call) fails, the host path gets its chance and reports what is really wrong
        log.debug("%s: host JPEG decode (%s)", path, exc)
        return None
    if r.buf is None:
        log.debug("%s: host JPEG decode (%s)", path, r.reason)
        return None
    return r
