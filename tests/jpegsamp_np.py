"""Baseline JPEG files whose chroma is subsampled 4:2:2 (luma sampling 2x1), 4:4:0 (1x2) or 4:1:1 (4x1), in NumPy and plain Python:
a restatement of what libjpeg's default decoder returns for them (and for gray, 4:4:4 and 4:2:0), and a writer, since Pillow writes
only 4:4:4, 4:2:2 and 4:2:0.

decode() is tests/jpegdec_np.py (marker walk, sequential Huffman decoding, islow IDCT, cropping, colour rows) with libjpeg's three
further upsamplers.  Each chroma plane is cropped to ceil(W h / hmax) x ceil(H v / vmax) first and the cropped edges replicate:
    h2v1 "fancy"   even output columns (3 s[c] + s[c-1] + 1) >> 2, odd ones (3 s[c] + s[c+1] + 2) >> 2, rows unchanged
    h1v2 "fancy"   even output rows    (3 s[r] + s[r-1] + 1) >> 2, odd ones (3 s[r] + s[r+1] + 2) >> 2, columns unchanged
    h4v1           plain replication: every sample serves four columns (libjpeg has no fancy filter for it)
write() is tests/jpegenc_np.py / tests/jpeg420_np.py (quantiser tables, integer DCT, Annex K Huffman coding, header) with a general
MCU: hs x vs luma blocks in raster order, then Cb, then Cr.  Its chroma downsample is a rounded box mean; the decoders under test do
not depend on it.  Nothing here shares code with gs360/ or with the kernels.
"""
import numpy as np

import jpeg420_np as enc420
import jpegdec_np as dec
import jpegenc_np as enc

SAMPLINGS = {"4:2:2": (2, 1), "4:4:0": (1, 2), "4:1:1": (4, 1)}


# ---- the decoder restated ----------------------------------------------------------------------------------------------------------
def _fancy(p, axis):
    """one axis doubled by libjpeg's triangle filter, the plane's edges replicated"""
    p = np.moveaxis(p.astype(np.int32), axis, 0)
    before, after = np.concatenate([p[:1], p[:-1]]), np.concatenate([p[1:], p[-1:]])
    out = np.empty((2 * p.shape[0],) + p.shape[1:], np.int32)
    out[0::2], out[1::2] = (3 * p + before + 1) >> 2, (3 * p + after + 2) >> 2
    return np.moveaxis(out, 0, axis)


def upsample_h2v1(p):
    """[h][w] -> [h][2w]"""
    return _fancy(p, 1)


def upsample_h1v2(p):
    """[h][w] -> [2h][w]"""
    return _fancy(p, 0)


def upsample_h4v1(p):
    """[h][w] -> [h][4w]"""
    return np.repeat(p.astype(np.int32), 4, axis=1)


UPSAMPLERS = {(1, 1): lambda p: p.astype(np.int32), (2, 2): dec.upsample_h2v2, (2, 1): upsample_h2v1, (1, 2): upsample_h1v2,
              (4, 1): upsample_h4v1}


def decode(data):
    """the bytes of a baseline JPEG file (gray, or Y sampled 1x1, 2x2, 2x1, 1x2 or 4x1 over 1x1 chroma) -> uint8 H x W or H x W x 3"""
    hd = dec.read_header(bytes(data))
    coef, cycle, (mw, mh, hmax, vmax) = dec.coefficients(hd)
    H, W, comps = hd["H"], hd["W"], hd["comps"]
    planes = []
    for c, (_i, h, v, tq) in enumerate(comps):
        if len(comps) == 1:
            h = v = 1
        nat = np.empty(64, np.int32)
        nat[dec.ZIGZAG] = hd["quant"][tq]
        idx = [b for b, cc in enumerate(cycle) if cc == c]
        px = dec.idct(coef.reshape(mw * mh, len(cycle), 64)[:, idx] * nat)
        plane = px.reshape(mh, mw, v, h, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(mh * v * 8, mw * h * 8)
        plane = plane[:-(-H * v // vmax), :-(-W * h // hmax)]
        assert hmax % h == 0 and vmax % v == 0
        planes.append(UPSAMPLERS[(hmax // h, vmax // v)](plane)[:H, :W].astype(np.int32))
    if len(planes) == 1:
        return planes[0].astype(np.uint8)
    y, cb, cr = planes[0], planes[1] - 128, planes[2] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


# ---- the writer --------------------------------------------------------------------------------------------------------------------
def _box(plane, hs, vs):
    """[H][W] (multiples of vs, hs) -> [H / vs][W / hs]: the rounded mean of every vs x hs cell"""
    H, W = plane.shape
    s = plane.reshape(H // vs, vs, W // hs, hs).sum(axis=(1, 3))
    return (s + hs * vs // 2) // (hs * vs)


def coefficients(img, hs, vs, quality):
    """H x W x 3 uint8 -> int64 [MCUs][hs vs + 2][64], zig-zag: the luma blocks of every 8 hs x 8 vs MCU in raster order, Cb, Cr"""
    a = np.asarray(img)
    p = enc.planes(a)                                                             # padded to multiples of 8; now to whole MCUs
    p = np.pad(p, ((0, 0), (0, -p.shape[1] % (8 * vs)), (0, -p.shape[2] % (8 * hs))), mode="edge")
    my, mx = p.shape[1] // (8 * vs), p.shape[2] // (8 * hs)
    qt = np.array(enc.quant_tables(quality), np.int64).reshape(2, 8, 8)
    z = np.empty((my, mx, hs * vs + 2, 64), np.int64)
    yb = p[0].reshape(my, vs, 8, mx, hs, 8).transpose(0, 3, 1, 4, 2, 5)           # [my][mx][block row][block column][y][x]
    z[:, :, :hs * vs] = enc420._quantised(yb, qt[0]).reshape(my, mx, hs * vs, 64)
    for k in (1, 2):
        z[:, :, hs * vs + k - 1] = enc420._quantised(_box(p[k], hs, vs).reshape(my, 8, mx, 8).transpose(0, 2, 1, 3), qt[1])
    return z.reshape(my * mx, hs * vs + 2, 64)


def scan(z, hs, vs, restart):
    """[MCUs][blocks][64] -> the entropy-coded segment with the Annex K tables; restart = MCUs per interval, 0 = no markers"""
    codes = [enc.huff_codes(t) for t in enc420.STANDARD]
    comp_of = [0] * (hs * vs) + [1, 2]
    n = len(z)
    per = restart if restart else n
    n_int = -(-n // per)
    out = bytearray()
    for k in range(n_int):
        w = enc.BitWriter()
        pred = [0, 0, 0]
        for m in range(k * per, min(n, (k + 1) * per)):
            for i, c in enumerate(comp_of):
                t = 2 if c else 0
                enc.encode_block(w, z[m, i], pred[c], codes[t], codes[t + 1])
                pred[c] = int(z[m, i, 0])
        w.pad()
        out += w.out
        if k + 1 < n_int:
            out += bytes([0xFF, 0xD0 + (k & 7)])
    return bytes(out)


def header(H, W, hs, vs, quality, restart):
    """tests/jpegenc_np.py's header with component 1's sampling byte patched, and without its DRI segment when restart is 0"""
    head = enc.header(H, W, 3, quality, restart if restart else 1)
    at = head.index(b"\xff\xc0") + 10                # marker, length, precision, H, W, Nf -> component 1's id
    assert head[at:at + 3] == b"\x01\x11\x00"
    head = head[:at + 1] + bytes([hs << 4 | vs]) + head[at + 2:]
    if not restart:
        dri = head.index(b"\xff\xdd\x00\x04")
        head = head[:dri] + head[dri + 6:]
    return head


def write(img, hs, vs, quality=90, restart=0):
    """H x W x 3 uint8 -> a whole JFIF file whose luma is sampled hs x vs over 1 x 1 chroma"""
    a = np.asarray(img)
    assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3 and 0 <= restart <= 65535
    return header(a.shape[0], a.shape[1], hs, vs, quality, restart) + scan(coefficients(a, hs, vs, quality), hs, vs, restart) + b"\xff\xd9"
