"""JPG-SPEC v1 restated in NumPy and plain Python: planes, quantised coefficients, the bit writer with restart
intervals, and the JFIF header.  Independent of gs360/jpegenc.py and of the HIP kernels: the tests compare both against this.
decode_scan reads a scan back with nothing but the header's own DHT and DRI segments, so the bit writer is pinned as well."""
import math

import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]

# Annex K.1 (natural order)
Q_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
          18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
Q_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32

# Annex K.3: (BITS[1..16], HUFFVAL)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
    0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
    0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
    0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa])


def _check_args(C, quality, restart):
    if C not in (1, 3):
        raise ValueError("C must be 1 or 3")
    if not 1 <= int(quality) <= 100:
        raise ValueError("quality must be in 1..100")
    if not 1 <= int(restart) <= 65535:
        raise ValueError("restart interval must be in 1..65535")


def quant_tables(quality):
    """-> [luma, chroma], 64 entries each in natural order: IJG's scaling of the Annex K tables"""
    q = int(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return [[min(max((b * s + 50) // 100, 1), 255) for b in base] for base in (Q_LUMA, Q_CHROMA)]


def huff_codes(table):
    """(BITS, HUFFVAL) -> {symbol: (code, length)} (Annex C)"""
    bits, vals = table
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def dct_matrix():
    a = np.empty((8, 8), np.int64)
    for u in range(8):
        k = 1.0 / math.sqrt(2.0) if u == 0 else 1.0
        for x in range(8):
            a[u, x] = int(round(2 ** 14 * k / 2.0 * math.cos((2 * x + 1) * u * math.pi / 16.0)))
    return a


def planes(img):
    """H x W (x C) uint8 -> int64 [C][H8][W8]: Y / Cb / Cr (or the sample), padded by repeating the last column and row, minus 128"""
    a = np.asarray(img)
    if a.ndim == 2:
        a = a[:, :, None]
    assert a.dtype == np.uint8 and a.shape[2] in (1, 3)
    v = a.astype(np.int64)
    if a.shape[2] == 1:
        p = [v[:, :, 0]]
    else:
        R, G, B = v[:, :, 0], v[:, :, 1], v[:, :, 2]
        p = [(19595 * R + 38470 * G + 7471 * B + 32768) >> 16,
             (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16,
             (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16]
    H, W = a.shape[:2]
    p = np.stack(p)
    assert p.min() >= 0 and p.max() <= 255
    p = np.pad(p, ((0, 0), (0, -H % 8), (0, -W % 8)), mode="edge")
    return p - 128


def coefficients(img, quality):
    """-> int64 [blocks_y][blocks_x][C][64]: quantised coefficients in zig-zag order"""
    p = planes(img)
    C, H8, W8 = p.shape
    s = p.reshape(C, H8 // 8, 8, W8 // 8, 8).transpose(1, 3, 0, 2, 4)            # [by][bx][c][y][x]
    A = dct_matrix()
    t1 = (np.einsum("ux,...yx->...yu", A, s) + 1024) >> 11
    assert np.abs(np.einsum("ux,...yx->...yu", A, s)).max() < 2 ** 31
    acc = np.einsum("vy,...yu->...vu", A, t1)
    assert np.abs(acc).max() + 65536 < 2 ** 31
    c = (acc + 65536) >> 17                                                      # [by][bx][c][v][u]
    qt = np.array(quant_tables(quality), np.int64).reshape(2, 8, 8)
    Q = qt[[0, 1, 1][:C]]                                                        # per component
    qc = np.sign(c) * ((np.abs(c) + (Q >> 1)) // Q)
    z = qc.reshape(qc.shape[:3] + (64,))[..., ZIGZAG]
    assert np.abs(z[..., 1:]).max(initial=0) <= 1023 and z[..., 0].min() >= -1024 and z[..., 0].max() <= 1016
    return z


class BitWriter:
    """MSB-first bits into bytes, 0x00 stuffed after every 0xFF"""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, code, length):
        assert 0 <= code < (1 << length)
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def pad(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _value_bits(v):
    """-> (size, bits) of a DC difference or AC coefficient (F.1.2.1)"""
    size = int(abs(v)).bit_length()
    return size, (v if v >= 0 else v + (1 << size) - 1)


def encode_block(w, z, pred, dc_codes, ac_codes):
    size, bits = _value_bits(int(z[0]) - pred)
    w.put(*dc_codes[size])
    if size:
        w.put(bits, size)
    run = 0
    for k in range(1, 64):
        v = int(z[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            w.put(*ac_codes[0xF0])
            run -= 16
        size, bits = _value_bits(v)
        w.put(*ac_codes[(run << 4) | size])
        w.put(bits, size)
        run = 0
    if run:
        w.put(*ac_codes[0x00])


def scan_from_coefficients(z, restart=8):
    """[by][bx][C][64] -> the entropy-coded scan: intervals of `restart` MCUs, RSTm between them, the last one padded as well"""
    by, bx, C, _ = z.shape
    mcus = z.reshape(by * bx, C, 64)
    dc = [huff_codes(DC_LUMA), huff_codes(DC_CHROMA), huff_codes(DC_CHROMA)]
    ac = [huff_codes(AC_LUMA), huff_codes(AC_CHROMA), huff_codes(AC_CHROMA)]
    out = bytearray()
    n = len(mcus)
    n_int = (n + restart - 1) // restart
    for k in range(n_int):
        w = BitWriter()
        pred = [0] * C
        for m in range(k * restart, min(n, (k + 1) * restart)):
            for c in range(C):
                encode_block(w, mcus[m, c], pred[c], dc[c], ac[c])
                pred[c] = int(mcus[m, c, 0])
        w.pad()
        out += w.out
        if k + 1 < n_int:
            out += bytes([0xFF, 0xD0 + (k & 7)])
    return bytes(out)


def scan(img, quality=100, restart=8):
    a = np.asarray(img)
    _check_args(1 if a.ndim == 2 else a.shape[2], quality, restart)
    return scan_from_coefficients(coefficients(a, quality), restart)


def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def header(H, W, C, quality, restart):
    """SOI, APP0 (JFIF 1.01, density 1:1), one DQT per table, SOF0, one DHT per table, DRI, SOS"""
    _check_args(C, quality, restart)
    assert 1 <= H <= 65535 and 1 <= W <= 65535
    qt = quant_tables(quality)
    h = bytearray(b"\xff\xd8")
    h += _seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(1 if C == 1 else 2):
        h += _seg(0xDB, bytes([t]) + bytes(qt[t][ZIGZAG[i]] for i in range(64)))
    sof = bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([C])
    for c in range(C):
        sof += bytes([c + 1, 0x11, 0 if c == 0 else 1])
    h += _seg(0xC0, sof)
    tables = [(0x00, DC_LUMA), (0x10, AC_LUMA)] + ([(0x01, DC_CHROMA), (0x11, AC_CHROMA)] if C == 3 else [])
    for tc_th, (bits, vals) in tables:
        h += _seg(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    h += _seg(0xDD, int(restart).to_bytes(2, "big"))
    sos = bytes([C])
    for c in range(C):
        sos += bytes([c + 1, 0x00 if c == 0 else 0x11])
    h += _seg(0xDA, sos + bytes([0, 63, 0]))
    return bytes(h)


def encode(img, quality=100, restart=8):
    """a whole JFIF file"""
    a = np.asarray(img)
    H, W = a.shape[:2]
    C = 1 if a.ndim == 2 else a.shape[2]
    return header(H, W, C, quality, restart) + scan(a, quality, restart) + b"\xff\xd9"


# ---- an independent decoder: pins the restatement's own bit stream -----------------------------------------------------------------
def _header_tables(header_bytes):
    """-> ({(class, id): {code as a bit string: symbol}}, restart interval, [(dc id, ac id) per scan component]) from the DHT, DRI and SOS
    segments of a header (T.81 B.2.4.2, B.2.4.4, B.2.3); the codes are generated from BITS and HUFFVAL as in Annex C"""
    h = bytes(header_bytes)
    assert h[:2] == b"\xff\xd8"
    p, tables, restart, comps = 2, {}, 0, None
    while comps is None:
        assert h[p] == 0xFF, "marker expected"
        marker, n = h[p + 1], int.from_bytes(h[p + 2:p + 4], "big")
        body = h[p + 4:p + 2 + n]
        p += 2 + n
        if marker == 0xC4:
            q = 0
            while q < len(body):
                tc_th, bits = body[q], body[q + 1:q + 17]
                vals = body[q + 17:q + 17 + sum(bits)]
                q += 17 + sum(bits)
                lut, code, k = {}, 0, 0
                for length in range(1, 17):
                    for _ in range(bits[length - 1]):
                        lut[f"{code:0{length}b}"] = vals[k]
                        code += 1
                        k += 1
                    code <<= 1
                tables[(tc_th >> 4, tc_th & 15)] = lut
        elif marker == 0xDD:
            restart = int.from_bytes(body, "big")
        elif marker == 0xDA:
            comps = [(body[2 + 2 * c] >> 4, body[2 + 2 * c] & 15) for c in range(body[0])]
    assert p == len(h), "the header ends with SOS"
    return tables, restart, comps


class _BitReader:
    """MSB-first bits of one restart interval's bytes, already unstuffed (kept as a string of 0s and 1s)"""

    def __init__(self, data):
        self.s, self.pos = "".join(f"{b:08b}" for b in data), 0

    def bits(self, n):
        if self.pos + n > len(self.s):
            raise ValueError("the interval's bits ran out")
        self.pos += n
        return int(self.s[self.pos - n:self.pos], 2) if n else 0

    def symbol(self, lut):
        for length in range(1, 17):
            v = lut.get(self.s[self.pos:self.pos + length])
            if v is not None and self.pos + length <= len(self.s):
                self.pos += length
                return v
        raise ValueError(f"no Huffman code matches at bit {self.pos}")

    def value(self, size):
        """EXTEND (F.2.2.1)"""
        v = self.bits(size)
        return v if size == 0 or v >> (size - 1) else v - (1 << size) + 1


def decode_scan(header_bytes, scan_bytes, n_mcu, C):
    """Baseline Huffman decoding (T.81 F.2.2) of an entropy-coded scan with the tables, restart interval and component selectors found
    in `header_bytes` alone -> int [n_mcu][C][64] zig-zag coefficients.  Checks what a strict decoder checks: every 0xFF is followed by
    0x00 or by the RSTm that is due, nothing follows the last MCU but 1-padding, no run passes coefficient 63.  ValueError otherwise."""
    tables, restart, comps = _header_tables(header_bytes)
    if len(comps) != C:
        raise ValueError(f"the header's scan has {len(comps)} components, not {C}")
    if restart < 1:
        raise ValueError("no DRI segment")
    data = bytes(scan_bytes)
    n_int = (n_mcu + restart - 1) // restart
    out = np.zeros((n_mcu, C, 64), np.int64)
    p = 0
    for k in range(n_int):
        body = bytearray()
        while p < len(data):                                      # this interval's bytes, unstuffed, up to its marker
            b = data[p]
            if b != 0xFF:
                body.append(b)
                p += 1
                continue
            if p + 1 >= len(data):
                raise ValueError(f"interval {k}: 0xFF ends the scan")
            if data[p + 1] == 0x00:
                body.append(0xFF)
                p += 2
                continue
            if k + 1 < n_int and data[p + 1] == 0xD0 + (k & 7):
                p += 2
                break
            raise ValueError(f"interval {k}: unexpected marker 0xFF{data[p + 1]:02X} at byte {p}")
        else:
            if k + 1 < n_int:
                raise ValueError(f"interval {k}: the scan ends before RST{k & 7}")
        r = _BitReader(body)
        pred = [0] * C
        try:
            for m in range(k * restart, min(n_mcu, (k + 1) * restart)):
                for c, (td, ta) in enumerate(comps):
                    pred[c] += r.value(r.symbol(tables[(0, td)]))
                    out[m, c, 0] = pred[c]
                    i = 1
                    while i < 64:
                        rs = r.symbol(tables[(1, ta)])
                        run, size = rs >> 4, rs & 15
                        if size == 0:
                            if run == 15:
                                i += 16
                                if i > 63:
                                    raise ValueError("a ZRL passes coefficient 63")
                                continue
                            if run:
                                raise ValueError(f"symbol 0x{rs:02X} in a baseline scan")
                            break
                        i += run
                        if i > 63:
                            raise ValueError("a run passes coefficient 63")
                        out[m, c, i] = r.value(size)
                        i += 1
        except ValueError as e:
            raise ValueError(f"interval {k}: {e}") from None
        rest = 8 * len(body) - r.pos
        if rest >= 8 or r.bits(rest) != (1 << rest) - 1:
            raise ValueError(f"interval {k}: {rest} bits follow its last MCU and are not 1-padding of the last byte")
    if p != len(data):
        raise ValueError(f"{len(data) - p} bytes follow the last interval")
    return out


def first_difference(header_bytes, got, want, n_mcu, C):
    """a sentence on where two scans of the same image part: the first differing MCU, component, zig-zag index and interval of the
    decoded coefficients, or the decoder's complaint about `got`"""
    at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    where = f"{len(got)} bytes against {len(want)}, first differing byte {at}"
    _t, restart, _c = _header_tables(header_bytes)
    zw = decode_scan(header_bytes, want, n_mcu, C)
    try:
        zg = decode_scan(header_bytes, got, n_mcu, C)
    except ValueError as e:
        return f"{where}; the stream does not decode: {e}"
    bad = np.argwhere(zg != zw)
    if not len(bad):
        return f"{where}; both decode to the same coefficients (padding, stuffing or markers differ)"
    m, c, i = (int(v) for v in bad[0])
    return (f"{where}; first differing coefficient: MCU {m} (interval {m // restart}), component {c}, zig-zag index {i}: "
            f"{int(zg[m, c, i])} against {int(zw[m, c, i])}")


# ---- the inputs the JPEG tests share ---------------------------------------------------------------------------------------------
def noise_image(h=37, w=53, c=3, seed=20261017):
    """seeded uniform noise: every coefficient busy, many stuffed bytes at quality 100"""
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, c) if c > 1 else (h, w), dtype=np.uint8)


def photo_image(h=75, w=100, seed=20261018):
    """photo-like RGB: sinusoids + a 16-pixel checker + sigma 6 noise (long zero runs and ZRLs at quality 75)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    img = np.stack([128 + 60 * np.sin(xx / 9.0 + c) + 40 * np.cos(yy / 7.0 - c) + 30 * (((xx // 16) + (yy // 16)) % 2) for c in range(3)], -1)
    return np.clip(np.rint(img + rng.normal(0.0, 6.0, img.shape)), 0, 255).astype(np.uint8)


def gray_of(img):
    v = img.astype(np.int64)
    return ((v[..., 0] * 4899 + v[..., 1] * 9617 + v[..., 2] * 1868 + 8192) >> 14).astype(np.uint8)


def checker_image(h=24, w=40):
    """one-pixel black / white checker: the largest coefficients"""
    yy, xx = np.mgrid[:h, :w]
    return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
