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

from . import capi

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


def assemble(H, W, C, bps, deflated, adler):
    """the whole file around a deflate stream: signature, IHDR (non-interlaced, colour type 0 / 2 / 6), one IDAT, IEND"""
    idat = ZLIB_HEADER + bytes(deflated) + struct.pack(">I", adler)
    ihdr = struct.pack(">IIBBBBB", int(W), int(H), 8 * int(bps), _COLOUR_TYPE[int(C)], 0, 0, 0)
    return SIGNATURE + _png_chunk(b"IHDR", ihdr) + _png_chunk(b"IDAT", idat) + _png_chunk(b"IEND", b"")


def deflate_items(ctx, items, take, give, slot=0, raw_capacity=True):
    """(the caller holds `slot`) items: [(DeviceBuffer or device address, H, W, C, bps, src_stride)] device images -> [(DeviceBuffer
    holding the deflate stream, its length, its Adler-32)].  One gs360_png_deflate call on `slot` encodes them all where they are; the
    lengths and the chunks' Adler sums (8 bytes per 64 KiB) come back.  raw_capacity: a stream gets the image's raw size plus a
    chunk header's worth, and one that needs more (noise) is coded again, alone, into a buffer of the bound; otherwise every stream
    gets the bound at once.  Device memory comes from take(nbytes) and goes back through give(buffer): everything taken but the stream
    buffers returned is given back before this returns or raises; those are the caller's to give back."""
    n = len(items)
    if not n:
        return []
    taken, kept = [], []

    def room(nbytes):
        taken.append(take(nbytes))
        return taken[-1]

    def run(jobs):
        counts = [n_chunks(H, W, C, bps) for _s, H, W, C, bps, _st, _o, _c in jobs]
        d_len, d_adler = room(8 * len(jobs)), room(8 * sum(counts))
        ctx.png_deflate_dev(jobs, d_len, d_adler, slot)
        lengths = [int(v) for v in ctx.download(d_len, (len(jobs),), np.uint64, slot)]
        sums = ctx.download(d_adler, (sum(counts), 2), np.uint32, slot)
        adlers, at = [], 0
        for (_s, H, W, C, bps, _st, _o, _c), cnt in zip(jobs, counts):
            adlers.append(adler_combine(sums[at:at + cnt], filtered_bytes(H, W, C, bps)))
            at += cnt
        return lengths, adlers
    try:
        caps = [min(bound(H, W, C, bps), H * W * C * bps + 4096) if raw_capacity else bound(H, W, C, bps) for _s, H, W, C, bps, _st in items]
        jobs = [(src, H, W, C, bps, stride, room(cap), cap) for (src, H, W, C, bps, stride), cap in zip(items, caps)]
        lengths, adlers = run(jobs)
        for i, length in enumerate(lengths):
            if length != capi.PNG_OVERFLOW:
                continue
            src, H, W, C, bps, stride = items[i]
            full = bound(H, W, C, bps)
            if full <= caps[i]:
                raise capi.Gs360Error(-2, "the PNG stream did not fit its bound")
            jobs[i] = (src, H, W, C, bps, stride, room(full), full)
            (lengths[i],), _ = run([jobs[i]])
            if lengths[i] == capi.PNG_OVERFLOW:
                raise capi.Gs360Error(-2, "the PNG stream did not fit its bound")
        kept = [job[6] for job in jobs]
        return list(zip(kept, lengths, adlers))
    finally:
        for b in taken:
            if not any(b is k for k in kept):
                give(b)


def encode_buffers(ctx, items, slot=0, raw_capacity=True):
    """(the caller holds `slot`) items: [(DeviceBuffer, H, W, C, bps, src_stride)] device images -> [bytes], one whole PNG file each:
    deflate_items with the context's own allocator, then each stream's bytes come back and get their zlib and PNG framing."""
    streams = deflate_items(ctx, items, ctx.alloc, ctx.free, slot, raw_capacity)
    try:
        return [assemble(H, W, C, bps, ctx.download(d, (length,), np.uint8, slot).tobytes(), adler)
                for (_s, H, W, C, bps, _st), (d, length, adler) in zip(items, streams)]
    finally:
        for d, _length, _adler in streams:
            ctx.free(d)


def encode_device(ctx, images, slot=0):
    """images: uint8 / uint16 ndarrays (H x W or H x W x C, C = 1, 3 or 4) or (DeviceBuffer, H, W, C, bps, src_stride) tuples of device
    images -> [bytes], one whole PNG file each.  One gs360_png_deflate call encodes them all; only the compressed bytes and 8 bytes of
    checksum per 64 KiB come back from the device."""
    items, owned = [], []
    try:
        for im in images:
            if isinstance(im, tuple):
                items.append(im)
                continue
            a = np.ascontiguousarray(im)
            if a.dtype not in (np.uint8, np.uint16):
                raise ValueError("PNG images are uint8 or uint16")
            H, W = a.shape[:2]
            buf = ctx.to_device(a, slot)
            owned.append(buf)
            items.append((buf, H, W, 1 if a.ndim == 2 else a.shape[2], a.dtype.itemsize, 0))
        with ctx.slot_locks[slot]:
            return encode_buffers(ctx, items, slot, raw_capacity=False)
    finally:
        for b in owned:
            ctx.free(b)
