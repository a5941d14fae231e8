"""PNG files from images resident on the device (PNG-SPEC v1).

The device writes the raw deflate stream of the filtered scanlines (gs360_png_deflate: per-row filter choice, one dynamic-Huffman block
per 64 KiB chunk, matches at three fixed distances) and each chunk's Adler-32 partial sums; this module folds those into the zlib
trailer, computes the IDAT CRC and writes signature, IHDR, one IDAT chunk and IEND.  It stands in for the host PNG writers of
gs360/imageio.py (Pillow at compress_level 3 for 8 bits, the filter-0 writer for 16), which compress on one host thread per view.
"""
import ctypes as ct
import os
import struct
import zlib

import numpy as np

from . import capi, devcodec

SIGNATURE = b"\x89PNG\r\n\x1a\n"
ZLIB_HEADER = b"\x78\x01"            # deflate, 32 KiB window, no preset dictionary, "fastest" level hint
CHUNK = capi.PNG_CHUNK
_ADLER = 65521
_COLOUR_TYPE = {1: 0, 3: 2, 4: 6}


def mode_from_env():
    """-> True when the device writes the `.png` files.  GS360_PNG_ENCODER = host (default: the host codecs write every file exactly
    as before) | device."""
    mode = os.environ.get("GS360_PNG_ENCODER", "host")
    if mode not in ("host", "device"):
        raise ValueError(f"GS360_PNG_ENCODER must be host or device (got {mode!r})")
    return mode == "device"


def filtered_bytes(H, W, C, bps):
    return int(H) * (1 + int(W) * int(C) * int(bps))


def n_chunks(H, W, C, bps):
    return -(-filtered_bytes(H, W, C, bps) // CHUNK)


def bound(H, W, C, bps):
    """bytes that hold any deflate stream of an H x W x C image of bps bytes per sample (gs360_png_bound)"""
    n = ct.c_size_t(0)
    L = capi.load_library()
    capi._check(L.gs360_png_bound(int(H), int(W), int(C), int(bps), ct.byref(n)), L)
    return int(n.value)


def adler_combine(parts, total):
    """parts: the chunks' (sum of bytes, sum of (n - i) * byte i) mod 65521 in stream order, total: the stream's length -> Adler-32"""
    s1, s2, left = 1, 0, int(total)
    for a, b in parts:
        n = min(CHUNK, left)
        s2 = (s2 + n * s1 + int(b)) % _ADLER
        s1 = (s1 + int(a)) % _ADLER
        left -= n
    return (s2 << 16) | s1


def _png_chunk(tag, payload):
    return struct.pack(">I", len(payload)) + tag + payload + struct.pack(">I", zlib.crc32(tag + payload) & 0xFFFFFFFF)


def head(H, W, C, bps, length):
    """the file's bytes in front of a deflate stream of `length` bytes: signature, IHDR (non-interlaced, colour type 0 / 2 / 6) and the
    one IDAT chunk's length, tag and zlib header"""
    ihdr = struct.pack(">IIBBBBB", int(W), int(H), 8 * int(bps), _COLOUR_TYPE[int(C)], 0, 0, 0)
    return SIGNATURE + _png_chunk(b"IHDR", ihdr) + struct.pack(">I", len(ZLIB_HEADER) + int(length) + 4) + b"IDAT" + ZLIB_HEADER


def tail(deflated, adler):
    """the file's bytes behind the deflate stream: its Adler-32, the IDAT chunk's CRC (which runs over the stream) and IEND"""
    trailer = struct.pack(">I", adler)
    crc = zlib.crc32(trailer, zlib.crc32(deflated, zlib.crc32(b"IDAT" + ZLIB_HEADER)))
    return trailer + struct.pack(">I", crc & 0xFFFFFFFF) + _png_chunk(b"IEND", b"")


TAIL_BYTES = len(tail(b"", 0))


def assemble(H, W, C, bps, deflated, adler):
    """the whole file around a deflate stream"""
    return head(H, W, C, bps, len(deflated)) + bytes(deflated) + tail(deflated, adler)


def deflate_items(ctx, items, take, give, slot=0, raw_capacity=True):
    """(the caller holds `slot`) items: [(DeviceBuffer or device address, H, W, C, bps, src_stride)] device images -> [(DeviceBuffer
    holding the deflate stream, its length, its Adler-32)].  One gs360_png_deflate call on `slot` encodes them all where they are; the
    lengths and the chunks' Adler sums (8 bytes per 64 KiB) come back.  raw_capacity: a stream gets the image's raw size plus a
    chunk header's worth, and one that needs more (noise) is coded again, alone, into a buffer of the bound; otherwise every stream
    gets the bound at once.  Device memory comes from take(nbytes) and goes back through give(buffer): everything taken but the stream
    buffers returned is given back before this returns or raises; those are the caller's to give back."""
    def first(it):
        _s, H, W, C, bps, _st = it
        return min(bound(H, W, C, bps), H * W * C * bps + 4096) if raw_capacity else bound(H, W, C, bps)

    def start(room):                                     # (the whole call's Adler buffer holds any single job's sums)
        d_len, d_adler = room(8 * len(items)), room(8 * sum(n_chunks(*it[1:5]) for it in items))

        def run(jobs):
            counts = [n_chunks(*job[1:5]) for job in jobs]
            ctx.png_deflate_dev(jobs, d_len, d_adler, slot)
            lengths = [int(v) for v in ctx.download(d_len, (len(jobs),), np.uint64, slot)]
            sums = ctx.download(d_adler, (sum(counts), 2), np.uint32, slot)
            ends = np.cumsum(counts)
            return lengths, [adler_combine(sums[end - cnt:end], filtered_bytes(*job[1:5])) for job, cnt, end in zip(jobs, counts, ends)]
        return run
    return devcodec.code_items(items, take, give, first, lambda it: bound(*it[1:5]), lambda it, out, cap: (*it, out, cap), start,
                               capi.PNG_OVERFLOW, "PNG stream")


def encode_buffers(ctx, items, slot=0, raw_capacity=True):
    """(the caller holds `slot`) items: [(DeviceBuffer, H, W, C, bps, src_stride)] device images -> [bytes], one whole PNG file each:
    deflate_items with the context's own allocator, then each stream's bytes come back and get their zlib and PNG framing."""
    streams = deflate_items(ctx, items, ctx.alloc, ctx.free, slot, raw_capacity)
    return devcodec.files_of(ctx, items, streams, lambda it, deflated, adler: assemble(*it[1:5], deflated, adler), slot)


def encode_device(ctx, images, slot=0):
    """images: uint8 / uint16 ndarrays (H x W or H x W x C, C = 1, 3 or 4) or (DeviceBuffer, H, W, C, bps, src_stride) tuples of device
    images -> [bytes], one whole PNG file each.  One gs360_png_deflate call encodes them all; only the compressed bytes and 8 bytes of
    checksum per 64 KiB come back from the device."""
    def as_item(im):
        a = np.ascontiguousarray(im)
        if a.dtype not in (np.uint8, np.uint16):
            raise ValueError("PNG images are uint8 or uint16")
        return a, (a.shape[0], a.shape[1], 1 if a.ndim == 2 else a.shape[2], a.dtype.itemsize, 0)
    return devcodec.encode_images(ctx, images, as_item, lambda items: encode_buffers(ctx, items, slot, raw_capacity=False), slot)
