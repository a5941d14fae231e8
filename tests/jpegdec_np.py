"""NumPy restatement of JPD-SPEC v1: a baseline JPEG file -> the pixels libjpeg's default decoder returns.

Sequential Huffman decoding bit by bit, then the arithmetic of section 12 on whole planes: dequantisation, the `jidctint` inverse DCT
(CONST_BITS 13, PASS1_BITS 2), planes cropped to ceil(W h / hmax) x ceil(H v / vmax), "fancy" h2v2 upsampling and the fixed-point
YCbCr -> RGB rows.  It has its own marker walk and shares no code with gs360/jpegdec.py or the kernels.  decode() raises Corrupt
where the stream has an invalid code, too few or too many bits for its blocks; the tests compare its output with Pillow's.
"""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


class Corrupt(ValueError):
    pass


def read_header(data):
    """-> dict(H, W, comps [(id, h, v, tq)], quant {id: 64 zig-zag}, huff {(class, id): (bits, vals)}, restart, sel [(td, ta)], scan)"""
    hd = {"quant": {}, "huff": {}, "restart": 0}
    at = 2
    while True:
        assert data[at] == 0xFF, "marker expected"
        m = data[at + 1]
        n = (data[at + 2] << 8) | data[at + 3]
        body = data[at + 4:at + 2 + n]
        if m == 0xC0:
            hd["H"], hd["W"] = (body[1] << 8) | body[2], (body[3] << 8) | body[4]
            hd["comps"] = [(body[6 + 3 * k], body[7 + 3 * k] >> 4, body[7 + 3 * k] & 15, body[8 + 3 * k]) for k in range(body[5])]
        elif m == 0xDB:
            for k in range(0, len(body), 65):
                hd["quant"][body[k] & 15] = np.frombuffer(body, np.uint8, 64, k + 1).astype(np.int32)
        elif m == 0xC4:
            k = 0
            while k < len(body):
                bits = list(body[k + 1:k + 17])
                hd["huff"][(body[k] >> 4, body[k] & 15)] = (bits, list(body[k + 17:k + 17 + sum(bits)]))
                k += 17 + sum(bits)
        elif m == 0xDD:
            hd["restart"] = (body[0] << 8) | body[1]
        elif m == 0xDA:
            hd["sel"] = [(body[2 + 2 * k] >> 4, body[2 + 2 * k] & 15) for k in range(body[0])]
            end = data.rfind(b"\xff\xd9")
            hd["scan"] = data[at + 2 + n:end]
            return hd
        at += 2 + n


def code_table(bits, vals):
    """{(length, code): symbol} of a canonical Huffman table"""
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            out[(ln, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return out


class Bits:
    """the bits of one restart interval, 0xFF 0x00 unstuffed"""

    def __init__(self, seg):
        raw = np.frombuffer(seg, np.uint8)
        keep = np.ones(raw.size, bool)
        keep[1:] &= ~((raw[:-1] == 0xFF) & (raw[1:] == 0x00))
        self.bits = np.unpackbits(raw[keep])
        self.at = 0

    def bit(self):
        if self.at >= self.bits.size:
            raise Corrupt("out of bits")
        self.at += 1
        return int(self.bits[self.at - 1])

    def take(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, table):
        code = 0
        for ln in range(1, 17):
            code = (code << 1) | self.bit()
            if (ln, code) in table:
                return table[(ln, code)]
        raise Corrupt("invalid code")

    def at_end(self):
        return self.bits.size - self.at < 8


def extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def split_segments(scan):
    """the scan's bytes between its RSTn markers"""
    raw = np.frombuffer(scan, np.uint8)
    ff = np.flatnonzero(raw[:-1] == 0xFF)
    marks = ff[(raw[ff + 1] >= 0xD0) & (raw[ff + 1] <= 0xD7)]
    starts = [0] + [int(m) + 2 for m in marks]
    ends = [int(m) for m in marks] + [raw.size]
    return [scan[a:b] for a, b in zip(starts, ends)]


def coefficients(hd):
    """-> (int32 [blocks][64] natural order with absolute DC values, blocks per MCU, component of each block of an MCU)"""
    comps = hd["comps"]
    cycle = [c for c, (_i, h, v, _t) in enumerate(comps) for _ in range(h * v if len(comps) > 1 else 1)]
    hmax = max(c[1] for c in comps) if len(comps) > 1 else 1
    vmax = max(c[2] for c in comps) if len(comps) > 1 else 1
    mw, mh = -(-hd["W"] // (8 * hmax)), -(-hd["H"] // (8 * vmax))
    n_mcu = mw * mh
    ri = hd["restart"] or n_mcu
    tables = {k: code_table(*v) for k, v in hd["huff"].items()}
    segs = split_segments(hd["scan"])
    if len(segs) != -(-n_mcu // ri):
        raise Corrupt("restart intervals")
    out = np.zeros((n_mcu * len(cycle), 64), np.int32)
    for s, seg in enumerate(segs):
        rd = Bits(seg)
        pred = [0] * len(comps)
        for m in range(s * ri, min((s + 1) * ri, n_mcu)):
            for b, c in enumerate(cycle):
                td, ta = hd["sel"][c]
                blk = out[m * len(cycle) + b]
                size = rd.symbol(tables[(0, td)])
                if size > 15:
                    raise Corrupt("DC size")
                pred[c] += extend(rd.take(size), size)
                blk[0] = pred[c]
                z = 1
                while z < 64:
                    sym = rd.symbol(tables[(1, ta)])
                    r, size = sym >> 4, sym & 15
                    if size == 0:
                        if r != 15:
                            break
                        z += 16
                        continue
                    z += r
                    if z > 63:
                        raise Corrupt("run past the block")
                    blk[ZIGZAG[z]] = extend(rd.take(size), size)
                    z += 1
        if not rd.at_end():
            raise Corrupt("bits left over")
    return out, cycle, (mw, mh, hmax, vmax)


def _idct8(v, descale):
    """libjpeg's jidctint butterfly on axis 0 of an int32 [8][...] array"""
    v0, v1, v2, v3, v4, v5, v6, v7 = (v[k] for k in range(8))
    z1 = (v2 + v6) * 4433
    tmp2, tmp3 = z1 + v6 * -15137, z1 + v2 * 6270
    tmp0, tmp1 = (v0 + v4) * 8192, (v0 - v4) * 8192
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = v7, v5, v3, v1
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    half = np.int32(1 << (descale - 1))
    return np.stack([tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]) + half >> descale


def idct(blocks):
    """int32 [n][64] dequantised, natural order -> uint8 [n][8][8]"""
    with np.errstate(over="ignore"):
        w = blocks.reshape(-1, 8, 8).astype(np.int32)
        w = _idct8(w.transpose(1, 0, 2), 11)                 # columns: axis 0 = row index
        w = _idct8(w.transpose(2, 1, 0), 18)                 # rows: axis 0 = column index -> [col][n][row]
        return np.clip(w.transpose(1, 2, 0) + 128, 0, 255).astype(np.uint8)


def upsample_h2v2(p):
    """libjpeg's h2v2_fancy_upsample of a cropped plane [h][w] -> [2h][2w]"""
    p = p.astype(np.int32)
    up, dn = np.concatenate([p[:1], p[:-1]]), np.concatenate([p[1:], p[-1:]])
    rows = np.empty((2 * p.shape[0], p.shape[1]), np.int32)
    rows[0::2], rows[1::2] = 3 * p + up, 3 * p + dn
    left, right = np.concatenate([rows[:, :1], rows[:, :-1]], 1), np.concatenate([rows[:, 1:], rows[:, -1:]], 1)
    out = np.empty((rows.shape[0], 2 * rows.shape[1]), np.int32)
    out[:, 0::2], out[:, 1::2] = (3 * rows + left + 8) >> 4, (3 * rows + right + 7) >> 4
    return out


def decode(data):
    """the bytes of a baseline JPEG file (gray, 4:4:4 or 4:2:0) -> uint8 H x W (gray) or H x W x 3 (RGB)"""
    hd = read_header(bytes(data))
    coef, cycle, (mw, mh, hmax, vmax) = coefficients(hd)
    H, W, comps = hd["H"], hd["W"], hd["comps"]
    planes = []
    for c, (_i, h, v, tq) in enumerate(comps):
        if len(comps) == 1:
            h = v = 1
        nat = np.empty(64, np.int32)
        nat[ZIGZAG] = hd["quant"][tq]
        idx = [b for b, cc in enumerate(cycle) if cc == c]
        px = idct(coef.reshape(mw * mh, len(cycle), 64)[:, idx] * nat)           # [mcu * h*v][8][8]
        plane = px.reshape(mh, mw, v, h, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(mh * v * 8, mw * h * 8)
        ph, pw = -(-H * v // vmax), -(-W * h // hmax)
        plane = plane[:ph, :pw]
        if (h, v) != (hmax, vmax):
            assert (hmax, vmax, h, v) == (2, 2, 1, 1)
            plane = upsample_h2v2(plane)
        planes.append(plane[:H, :W].astype(np.int32))
    if len(planes) == 1:
        return planes[0].astype(np.uint8)
    y, cb, cr = planes[0], planes[1] - 128, planes[2] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)
