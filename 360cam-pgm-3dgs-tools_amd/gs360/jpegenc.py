"""Baseline JFIF files from images resident on the device (JPG-SPEC v1).

The device writes the entropy-coded scan (gs360_jpeg_scan_u8: YCbCr 4:4:4 or gray, the Annex K Huffman tables, restart intervals);
this module builds the header that describes it, appends EOI and offers the whole round trip for arrays and device buffers.  With
huffman="optimal" the device builds every image's own tables (gs360_jpeg_scan_opt_u8, the reference's `-huffman optimal`) and the
header's DHT segments carry those.  It stands in for the reference's image writer at PC:327-338 (ffmpeg's mjpeg encoder behind `-q:v`), which the host path leaves to Pillow.
"""
import ctypes as ct
import os

import numpy as np

from . import capi, devcodec

EOI = b"\xff\xd9"

_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
           35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
# ITU-T T.81 Annex K.1, natural order
_Q_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
           18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
_Q_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
# Annex K.3: BITS then HUFFVAL.  The AC value lists are regular: every (run, size) symbol, ordered by code length.
_DC_LUMA = bytes((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0)) + bytes(range(12))
_DC_CHROMA = bytes((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)) + bytes(range(12))
_AC_LUMA = bytes((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d)) + bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f0243362728209"
    "0a161718191a25262728292a3435363738393a434445464748494a535455565758595a636465"
    "666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9"
    "aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9ea"
    "f1f2f3f4f5f6f7f8f9fa")
_AC_CHROMA = bytes((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77)) + bytes.fromhex(
    "0001020311040521310612415107617113223281081442"
    "91a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445"
    "464748494a535455565758595a636465666768696a737475767778797a82838485868788898a"
    "92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3"
    "d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
assert len(_AC_LUMA) == len(_AC_CHROMA) == 16 + 162


def quality_for(jpeg_q):
    """ffmpeg's -q:v -> the quality imageio.write_image gives Pillow: None or 1 -> 100, >= 2 -> 95"""
    return 95 if (jpeg_q is not None and jpeg_q >= 2) else 100


def quant_tables(quality):
    """[luma, chroma] in natural order: IJG's scaling of the Annex K tables, forced to baseline (1..255)"""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError("quality must be in 1..100")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return [[min(max((b * s + 50) // 100, 1), 255) for b in base] for base in (_Q_LUMA, _Q_CHROMA)]


def _segment(marker, payload):
    return bytes((0xFF, marker)) + (len(payload) + 2).to_bytes(2, "big") + payload


TABLE_BYTES = 272            # GS360_JPEG_TABLE_BYTES: 16 BITS + up to 256 HUFFVAL, zero padded
HUFFMAN_MODES = ("standard", "optimal")
SUBSAMPLINGS = {"4:4:4": capi.JPEG_444, "4:2:0": capi.JPEG_420}      # -> GS360_JPEG_444 / GS360_JPEG_420 (Pillow's numbers)
RESTART = 8                  # MCUs per restart interval the engine and the dual-fisheye renderer ask for (JPG-SPEC v1's default)


def mode_from_env():
    """-> None (the host codecs write the views) or the device encoder's Huffman mode.  GS360_JPEG_ENCODER = host (default) | device and
    GS360_JPEG_HUFFMAN = standard (default: the Annex K tables) | optimal (every image's own tables, the reference's `-huffman
    optimal`; only meaningful with `device`)."""
    if os.environ.get("GS360_JPEG_ENCODER", "host") != "device":
        return None
    huffman = os.environ.get("GS360_JPEG_HUFFMAN", "standard")
    if huffman not in HUFFMAN_MODES:
        raise ValueError(f"GS360_JPEG_HUFFMAN must be standard or optimal (got {huffman!r})")
    return huffman


def _subsampling(name):
    if name not in SUBSAMPLINGS:
        raise ValueError("subsampling must be '4:4:4' or '4:2:0'")
    return SUBSAMPLINGS[name]


def header(H, W, C, quality, restart, tables=None, subsampling="4:4:4"):
    """Everything in front of the scan: SOI, APP0 (JFIF 1.01, density 1:1), DQT per table, SOF0, DHT per table, DRI, SOS.  `tables`: the
    4 * 272 bytes gs360_jpeg_scan_opt_u8 returned for the image (DC0, AC0, DC1, AC1); None: the Annex K tables.  subsampling="4:2:0"
    ("JPG-SPEC v1, 4:2:0"): component 1 of a colour image samples 2 x 2; a gray image's header does not change."""
    H, W, C, restart = int(H), int(W), int(C), int(restart)
    luma = 0x22 if _subsampling(subsampling) == capi.JPEG_420 else 0x11
    if C not in (1, 3):
        raise ValueError("C must be 1 or 3")
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError("JPEG sides are 1..65535")
    if not 1 <= restart <= 65535:
        raise ValueError("restart interval must be in 1..65535")
    qt = quant_tables(quality)
    n_tab = 1 if C == 1 else 2
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(n_tab):
        out += _segment(0xDB, bytes((t,)) + bytes(qt[t][z] for z in _ZIGZAG))
    sof = bytes((8,)) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes((C,))
    sos = bytes((C,))
    for c in range(C):
        sof += bytes((c + 1, luma if (c == 0 and C == 3) else 0x11, min(c, 1)))
        sos += bytes((c + 1, 0x11 * min(c, 1)))
    out += _segment(0xC0, sof)
    dht = (_DC_LUMA, _AC_LUMA, _DC_CHROMA, _AC_CHROMA)
    if tables is not None:
        tables = bytes(tables)
        if len(tables) != 4 * TABLE_BYTES:
            raise ValueError("tables must hold 4 x 272 bytes")
        dht = [tables[k * TABLE_BYTES:k * TABLE_BYTES + 16 + sum(tables[k * TABLE_BYTES:k * TABLE_BYTES + 16])] for k in range(4)]
    for ident, table in zip((0x00, 0x10, 0x01, 0x11)[:2 * n_tab], dht):
        out += _segment(0xC4, bytes((ident,)) + table)
    out += _segment(0xDD, restart.to_bytes(2, "big"))
    return out + _segment(0xDA, sos + b"\x00\x3f\x00")


def scan_bound(H, W, C, restart=8, subsampling="4:4:4"):
    """bytes that hold any scan of an H x W x C image (gs360_jpeg_scan_bound_sub)"""
    n = ct.c_size_t(0)
    L = capi.load_library()
    capi._check(L.gs360_jpeg_scan_bound_sub(int(H), int(W), int(C), int(restart), _subsampling(subsampling), ct.byref(n)), L)
    return int(n.value)


def scan_items(ctx, items, take, give, quality=100, restart=RESTART, slot=0, huffman="standard", subsampling="4:4:4", raw_capacity=True):
    """(the caller holds `slot`) items: [(DeviceBuffer, H, W, C)] tight 8-bit device images -> [(DeviceBuffer holding the scan, its
    length, its 4 x 272 table bytes or None)].  One gs360_jpeg_scan_sub_u8 call on `slot` encodes them all where they are; the lengths
    and, with "optimal", the tables (1 088 bytes an image) come back.  raw_capacity: a scan gets the image's raw size and one that
    needs more (noise at quality 100) is coded again, alone and in the same mode, into a buffer of the bound; otherwise every scan gets
    the bound at once.  Device memory comes from take(nbytes) and goes back through give(buffer): everything taken but the scan
    buffers returned is given back before this returns or raises; those are the caller's to give back.  The length and table
    buffers are taken at 8 and 1 088 bytes an item, so no batch is too large for them."""
    if huffman not in HUFFMAN_MODES:
        raise ValueError("huffman must be 'standard' or 'optimal'")
    sub = _subsampling(subsampling)
    optimal = huffman == "optimal"

    def start(room):
        d_len = room(8 * len(items))
        d_tab = room(4 * TABLE_BYTES * len(items)) if optimal else None

        def run(jobs):
            ctx.jpeg_scan_sub_dev(jobs, d_len, d_tab, quality=quality, restart=restart, subsampling=sub, slot=slot)
            tabs = ctx.download(d_tab, (len(jobs), 4 * TABLE_BYTES), np.uint8, slot) if optimal else [None] * len(jobs)
            return [int(v) for v in ctx.download(d_len, (len(jobs),), np.uint64, slot)], [None if t is None else t.tobytes() for t in tabs]
        return run

    def bound(item):
        return scan_bound(*item[1:], restart, subsampling)

    def raw_size(item):
        return item[1] * item[2] * item[3]
    return devcodec.code_items(items, take, give, raw_size if raw_capacity else bound, bound, lambda item, out, cap: (*item, 0, out, cap), start,
                               capi.JPEG_OVERFLOW, "JPEG scan")


def encode_buffers(ctx, items, quality=100, restart=8, slot=0, huffman="standard", subsampling="4:4:4", raw_capacity=True):
    """(the caller holds `slot`) items: [(DeviceBuffer, H, W, C)] tight 8-bit device images -> [bytes], one whole JFIF file each:
    scan_items with the context's own allocator, then each scan's bytes come back and get their header and EOI."""
    scans = scan_items(ctx, items, ctx.alloc, ctx.free, quality, restart, slot, huffman, subsampling, raw_capacity)
    return devcodec.files_of(ctx, items, scans, lambda it, scan, tab: header(*it[1:], quality, restart, tab, subsampling) + scan + EOI, slot)


def encode_device(ctx, images, quality=100, restart=8, slot=0, huffman="standard", subsampling="4:4:4"):
    """images: uint8 ndarrays (H x W or H x W x C) or (DeviceBuffer, H, W, C) tuples of tight device images -> [bytes], one whole
    JFIF file each.  One gs360_jpeg_scan_sub_u8 call (huffman="optimal": every image's own tables; subsampling="4:2:0": 2 x 2 chroma
    subsampling for colour images) encodes them all; only the scans' bytes, and with "optimal" 1 088 bytes of tables per image, come
    back from the device."""
    if huffman not in HUFFMAN_MODES:
        raise ValueError("huffman must be 'standard' or 'optimal'")
    _subsampling(subsampling)

    def as_item(im):
        a = np.ascontiguousarray(im, dtype=np.uint8)
        return a, (a.shape[0], a.shape[1], 1 if a.ndim == 2 else a.shape[2])
    return devcodec.encode_images(ctx, images, as_item,
                                  lambda items: encode_buffers(ctx, items, quality, restart, slot, huffman, subsampling, raw_capacity=False), slot)
