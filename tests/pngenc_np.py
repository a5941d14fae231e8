"""NumPy restatement of PNG-SPEC v1: the bytes the device PNG encoder must produce.

Written from the spec and from RFC 1951 / RFC 1950 / the PNG specification, not from the kernels: the filters run over whole arrays,
the match lengths come from run-length tables per candidate distance, the Huffman construction is a loop over arrays, and the length
and distance codes are looked up in RFC 1951's tables (the kernels compute them arithmetically).
"""
import struct
import zlib

import numpy as np

CHUNK = 65536          # filtered bytes per deflate block
SEGMENT = 512          # bytes one lane parses; no match crosses a segment's end
MAX_MATCH = 258
MIN_MATCH = 3
MAX_DIST = 32768
MAX_BITS = 15
N_LITLEN = 286
N_DIST = 30
SIGNATURE = b"\x89PNG\r\n\x1a\n"
ZLIB_HEADER = b"\x78\x01"
# RFC 1951 3.2.5: (first length, extra bits) of the length codes 257..285, (first distance, extra bits) of the distance codes 0..29
_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
              12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
_CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def _length_symbol(length):
    """-> (symbol, extra bits, extra value)"""
    k = max(i for i in range(29) if _LEN_BASE[i] <= length)
    return 257 + k, _LEN_EXTRA[k], length - _LEN_BASE[k]


def _distance_symbol(dist):
    k = max(i for i in range(30) if _DIST_BASE[i] <= dist)
    return k, _DIST_EXTRA[k], dist - _DIST_BASE[k]


# ---- filtering ------------------------------------------------------------------------------------------------------------------------
def image_bytes(img):
    """H x W [x C] uint8 / uint16 -> (H x W*bpp uint8 rows as PNG stores them: 16-bit samples big-endian, bpp, C, bit depth)"""
    a = np.asarray(img)
    if a.ndim == 2:
        a = a[:, :, None]
    if a.dtype not in (np.uint8, np.uint16) or a.shape[2] not in (1, 3, 4) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("PNG-SPEC v1 takes H x W x {1, 3, 4} uint8 or uint16")
    H, W, C = a.shape
    bps = a.dtype.itemsize
    rows = np.ascontiguousarray(a.astype(">u2" if bps == 2 else np.uint8)).view(np.uint8).reshape(H, W * C * bps)
    return rows, C * bps, C, 8 * bps


def filter_rows(rows, bpp):
    """-> (H x (1 + Wb) filtered stream, the rows' filter types, the 5 x H costs): all five types, smallest sum of |int8 residual|,
    ties to the lower"""
    H, Wb = rows.shape
    x = rows.astype(np.int32)
    a = np.zeros_like(x)
    a[:, bpp:] = x[:, :-bpp] if Wb > bpp else 0
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, bpp:] = x[:-1, :-bpp] if Wb > bpp else 0
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    res = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]).astype(np.uint8)          # 5 x H x Wb
    cost = np.abs(res.view(np.int8).astype(np.int32)).sum(axis=2)                              # 5 x H
    types = np.argmin(cost, axis=0)                                                            # first minimum: the lower type
    out = np.empty((H, 1 + Wb), np.uint8)
    out[:, 0] = types
    out[:, 1:] = res[types, np.arange(H)]
    return out, types, cost


# ---- parsing --------------------------------------------------------------------------------------------------------------------------
def candidate_distances(W, bpp):
    return [1, bpp, 1 + W * bpp]


def parse_chunk(data, dists):
    """data: one chunk of the filtered stream -> [(literal,) | (length, distance)] in stream order.  Greedy per segment: at each
    position the longest match of >= 3 bytes among the candidate distances (source inside the chunk, distance <= 32768, the match
    inside the segment, at most 258 bytes); ties go to the earlier candidate."""
    n = len(data)
    seg_end = np.minimum((np.arange(n) // SEGMENT + 1) * SEGMENT, n)
    runs = []
    for d in dists:
        run = np.zeros(n + 1, np.int64)
        if d <= min(n - 1, MAX_DIST):
            eq = np.zeros(n, bool)
            eq[d:] = data[d:] == data[:-d]
            # bytes equal to their source from q on: distance to the next unequal position
            idx = np.where(~eq, np.arange(n), n)
            nxt = np.minimum.accumulate(idx[::-1])[::-1]
            run[:n] = nxt - np.arange(n)
        runs.append(np.minimum(np.minimum(run[:n], seg_end - np.arange(n)), MAX_MATCH))
    runs = np.stack(runs)
    best_k = np.argmax(runs, axis=0)                       # first maximum: the earlier candidate
    best = runs[best_k, np.arange(n)]
    syms = []
    q = 0
    while q < n:
        if best[q] >= MIN_MATCH:
            syms.append((int(best[q]), int(dists[best_k[q]])))
            q += int(best[q])
        else:
            syms.append((int(data[q]),))
            q += 1
    return syms


# ---- code lengths ---------------------------------------------------------------------------------------------------------------------
def code_lengths(counts, info=None):
    """Symbol counts -> code lengths of at most 15 bits.  No symbol used: symbol 0 gets one bit.  One symbol used: it gets one bit.
    Otherwise Huffman's merges (the two smallest counts, ties to the LARGEST index; the sum stays at the smaller one's index), the
    counts of lengths above 15 folded down as T.81 K.3 does for 16, and the final lengths handed out in order of (unlimited length,
    symbol).  info (a dict) receives "unlimited": the deepest length before the fold."""
    counts = np.asarray(counts, np.int64)
    n = len(counts)
    out = np.zeros(n, np.int64)
    used = np.flatnonzero(counts)
    if len(used) <= 1:
        out[used[0] if len(used) else 0] = 1
        return out
    f = counts.copy()
    grp = np.arange(n)
    length = np.zeros(n, np.int64)
    idx = np.arange(n)
    big = np.iinfo(np.int64).max
    while True:
        key = np.where(f > 0, (f << 9) | (511 - idx), big)
        c1 = int(np.argmin(key))
        key[c1] = big
        c2 = int(np.argmin(key))
        if key[c2] == big:
            break
        f[c1] += f[c2]
        f[c2] = 0
        both = (counts > 0) & ((grp == c1) | (grp == c2))
        length[both] += 1
        grp[both] = c1
    if info is not None:
        info["unlimited"] = int(length.max())
    bits = np.bincount(length[length > 0], minlength=64).astype(np.int64)
    for i in range(len(bits) - 1, MAX_BITS, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    order = sorted(used, key=lambda s: (length[s], s))
    final = [ln for ln in range(1, MAX_BITS + 1) for _ in range(int(bits[ln]))]
    assert len(final) == len(order)
    for s, ln in zip(order, final):
        out[s] = ln
    return out


def canonical_codes(lengths):
    """RFC 1951 3.2.2 -> codes (MSB-first values)"""
    lengths = [int(v) for v in lengths]
    bl = [0] * (MAX_BITS + 2)
    for ln in lengths:
        bl[ln] += 1
    bl[0] = 0
    code, nxt = 0, [0] * (MAX_BITS + 2)
    for b in range(1, MAX_BITS + 1):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    codes = [0] * len(lengths)
    for s, ln in enumerate(lengths):
        if ln:
            codes[s] = nxt[ln]
            nxt[ln] += 1
    return codes


# ---- bit writing ----------------------------------------------------------------------------------------------------------------------
class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):                      # LSB first (header fields, extra bits)
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, nbits):                      # Huffman codes go MSB first
        self.put(int(format(code, "0%db" % nbits)[::-1], 2) if nbits else 0, nbits)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)


def deflate_chunk(data, dists, last):
    """one chunk -> one dynamic block and an empty stored block (BFINAL on the stream's last)"""
    syms = parse_chunk(data, dists)
    lit = np.zeros(N_LITLEN, np.int64)
    dst = np.zeros(N_DIST, np.int64)
    lit[256] = 1
    for s in syms:
        if len(s) == 1:
            lit[s[0]] += 1
        else:
            lit[_length_symbol(s[0])[0]] += 1
            dst[_distance_symbol(s[1])[0]] += 1
    ll, dl = code_lengths(lit), code_lengths(dst)
    lc, dc = canonical_codes(ll), canonical_codes(dl)
    w = _Bits()
    w.put(0, 1)
    w.put(2, 2)
    w.put(N_LITLEN - 257, 5)
    w.put(N_DIST - 1, 5)
    w.put(19 - 4, 4)
    for s in _CL_ORDER:                               # the fixed code-length code: symbols 0..15 at 4 bits, 16..18 unused
        w.put(4 if s < 16 else 0, 3)
    for ln in list(ll) + list(dl):
        w.code(int(ln), 4)
    for s in syms:
        if len(s) == 1:
            w.code(lc[s[0]], int(ll[s[0]]))
        else:
            sym, eb, ev = _length_symbol(s[0])
            w.code(lc[sym], int(ll[sym]))
            w.put(ev, eb)
            sym, eb, ev = _distance_symbol(s[1])
            w.code(dc[sym], int(dl[sym]))
            w.put(ev, eb)
    w.code(lc[256], int(ll[256]))
    w.put(1 if last else 0, 1)
    w.put(0, 2)
    w.align()
    return bytes(w.out) + b"\x00\x00\xff\xff"


def adler_partial(data):
    """-> (sum of the bytes, sum of (n - i) * byte i), both mod 65521: what the device reports per chunk"""
    d = np.frombuffer(bytes(data), np.uint8).astype(np.int64)
    n = len(d)
    return int(d.sum() % 65521), int((d * (n - np.arange(n))).sum() % 65521)


def adler_combine(parts):
    """[(s1 part, s2 part, length)] in stream order -> Adler-32"""
    s1, s2 = 1, 0
    for a, b, n in parts:
        s2 = (s2 + n * s1 + b) % 65521
        s1 = (s1 + a) % 65521
    return (s2 << 16) | s1


# ---- whole files ----------------------------------------------------------------------------------------------------------------------
def filtered_stream(img):
    rows, bpp, _C, _depth = image_bytes(img)
    return filter_rows(rows, bpp)[0].reshape(-1)


def deflate(img):
    """-> (the raw deflate bytes the device writes, the chunks' Adler partials [(a, b, length)])"""
    rows, bpp, _C, _depth = image_bytes(img)
    stream = filter_rows(rows, bpp)[0].reshape(-1)
    dists = candidate_distances(rows.shape[1] // bpp, bpp)
    out, parts = [], []
    for c0 in range(0, len(stream), CHUNK):
        data = stream[c0:c0 + CHUNK]
        out.append(deflate_chunk(data, dists, c0 + CHUNK >= len(stream)))
        parts.append(adler_partial(data) + (len(data),))
    return b"".join(out), parts


def _png_chunk(tag, payload):
    return struct.pack(">I", len(payload)) + tag + payload + struct.pack(">I", zlib.crc32(tag + payload) & 0xFFFFFFFF)


def assemble(H, W, C, depth, deflated, adler):
    idat = ZLIB_HEADER + deflated + struct.pack(">I", adler)
    ihdr = struct.pack(">IIBBBBB", W, H, depth, {1: 0, 3: 2, 4: 6}[C], 0, 0, 0)
    return SIGNATURE + _png_chunk(b"IHDR", ihdr) + _png_chunk(b"IDAT", idat) + _png_chunk(b"IEND", b"")


def encode(img):
    """-> the whole PNG file of PNG-SPEC v1"""
    rows, _bpp, C, depth = image_bytes(img)
    deflated, parts = deflate(img)
    return assemble(rows.shape[0], rows.shape[1] * 8 // (C * depth), C, depth, deflated, adler_combine(parts))


def idat_payload(png):
    """the concatenated IDAT payloads of a PNG file"""
    out, off = b"", 8
    while off < len(png):
        n, tag = struct.unpack(">I4s", png[off:off + 8])
        if tag == b"IDAT":
            out += png[off + 8:off + 8 + n]
        off += 12 + n
    return out
