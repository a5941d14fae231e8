""""JPG-SPEC v1, 4:2:0"  restated in NumPy and plain Python on top of tests/jpegenc_np.py and tests/jpegopt_np.py:
full-resolution planes padded to 16, libjpeg's h2v2 chroma downsample, 16 x 16 MCUs of six blocks, and the scan, header and file they
give with the Annex K tables or the image's own.  Independent of gs360/jpegenc.py and of the HIP kernels: the tests compare both
against this, and this against Pillow's decoder and Pillow's own `subsampling=2` files."""
import numpy as np

import jpegenc_np as ref
import jpegopt_np as opt

COMP_OF = (0, 0, 0, 0, 1, 2)          # the component of block i of an MCU: Y(0,0), Y(0,1), Y(1,0), Y(1,1), Cb, Cr


def is_gray(img):
    a = np.asarray(img)
    return a.ndim == 2 or a.shape[2] == 1


def downsample(plane):
    """[H][W] (both even) -> [H/2][W/2]: libjpeg's h2v2_downsample, (a + b + c + d + bias) >> 2 with bias 1 at even output columns
    and 2 at odd ones"""
    p = np.asarray(plane, np.int64)
    s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
    bias = 1 + (np.arange(s.shape[1]) & 1)
    return (s + bias[None, :]) >> 2


def planes(img):
    """H x W x 3 uint8 -> (Y int64 [H16][W16], Cb and Cr int64 [H16/2][W16/2]), all minus 128: v1's colour formulas at full resolution,
    the three planes padded to multiples of 16 by repeating the last column and row, chroma downsampled after the padding"""
    a = np.asarray(img)
    assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3
    v = a.astype(np.int64)
    R, G, B = v[:, :, 0], v[:, :, 1], v[:, :, 2]
    p = np.stack([(19595 * R + 38470 * G + 7471 * B + 32768) >> 16,
                  (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16,
                  (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16])
    assert p.min() >= 0 and p.max() <= 255
    H, W = a.shape[:2]
    p = np.pad(p, ((0, 0), (0, -H % 16), (0, -W % 16)), mode="edge")
    return p[0] - 128, downsample(p[1]) - 128, downsample(p[2]) - 128


def _quantised(s, Q):
    """[...][8][8] samples -> [...][64] quantised zig-zag coefficients: v1's two integer matrix products and quantiser"""
    A = ref.dct_matrix()
    t1 = (np.einsum("ux,...yx->...yu", A, s) + 1024) >> 11
    c = (np.einsum("vy,...yu->...vu", A, t1) + 65536) >> 17
    qc = np.sign(c) * ((np.abs(c) + (Q >> 1)) // Q)
    return qc.reshape(qc.shape[:-2] + (64,))[..., ref.ZIGZAG]


def coefficients(img, quality):
    """H x W x 3 -> int64 [mcus_y][mcus_x][6][64]: the six blocks of every 16 x 16 MCU in scan order, zig-zag"""
    Y, Cb, Cr = planes(img)
    my, mx = Y.shape[0] // 16, Y.shape[1] // 16
    qt = np.array(ref.quant_tables(quality), np.int64).reshape(2, 8, 8)
    yb = Y.reshape(my, 2, 8, mx, 2, 8).transpose(0, 3, 1, 4, 2, 5)               # [my][mx][block row][block column][y][x]
    z = np.empty((my, mx, 6, 64), np.int64)
    z[:, :, :4] = _quantised(yb, qt[0]).reshape(my, mx, 4, 64)
    for k, p in ((4, Cb), (5, Cr)):
        z[:, :, k] = _quantised(p.reshape(my, 8, mx, 8).transpose(0, 2, 1, 3), qt[1])
    return z


STANDARD = (ref.DC_LUMA, ref.AC_LUMA, ref.DC_CHROMA, ref.AC_CHROMA)


def scan_from_coefficients(z, restart=8, tables=STANDARD):
    """[my][mx][6][64] -> the entropy-coded scan: intervals of `restart` MCUs, DC prediction per component across the whole sequence
    (the four Y blocks chain), reset at each interval.  tables: [DC0, AC0, DC1, AC1] as (BITS, HUFFVAL)"""
    mcus = np.asarray(z).reshape(-1, 6, 64)
    codes = [ref.huff_codes(t) for t in tables]
    out = bytearray()
    n = len(mcus)
    n_int = (n + restart - 1) // restart
    for k in range(n_int):
        w = ref.BitWriter()
        pred = [0, 0, 0]
        for m in range(k * restart, min(n, (k + 1) * restart)):
            for i, c in enumerate(COMP_OF):
                t = 2 if c else 0
                ref.encode_block(w, mcus[m, i], pred[c], codes[t], codes[t + 1])
                pred[c] = int(mcus[m, i, 0])
        w.pad()
        out += w.out
        if k + 1 < n_int:
            out += bytes([0xFF, 0xD0 + (k & 7)])
    return bytes(out)


def symbol_hist(z, restart):
    """[my][mx][6][64] -> [DC0, AC0, DC1, AC1], 256 counts each: exactly the symbols scan_from_coefficients emits"""
    mcus = np.asarray(z).reshape(-1, 6, 64)
    hist = [[0] * 256 for _ in range(4)]
    pred = [0, 0, 0]
    for m in range(len(mcus)):
        if m % restart == 0:
            pred = [0, 0, 0]
        for i, c in enumerate(COMP_OF):
            t = 2 if c else 0
            blk = [int(v) for v in mcus[m, i]]
            hist[t][abs(blk[0] - pred[c]).bit_length()] += 1
            pred[c] = blk[0]
            run = 0
            for v in blk[1:]:
                if v == 0:
                    run += 1
                    continue
                hist[t + 1][0xF0] += run >> 4
                hist[t + 1][((run & 15) << 4) | abs(v).bit_length()] += 1
                run = 0
            if run:
                hist[t + 1][0x00] += 1
    return hist


def scan(img, quality=100, restart=8):
    """gray images have no chroma: their scan is v1's"""
    a = np.asarray(img)
    if is_gray(a):
        return ref.scan(a, quality, restart)
    ref._check_args(3, quality, restart)
    return scan_from_coefficients(coefficients(a, quality), restart)


def scan_optimal(img, quality=100, restart=8):
    """-> (scan, [DC0, AC0, DC1, AC1] as (BITS, HUFFVAL)): table 0 serves Y, table 1 Cb and Cr"""
    a = np.asarray(img)
    if is_gray(a):
        return opt.scan_optimal(a, quality, restart)
    ref._check_args(3, quality, restart)
    z = coefficients(a, quality)
    tables = [opt.optimal_table(h) for h in symbol_hist(z, restart)]
    return scan_from_coefficients(z, restart, tables), tables


def _sampled(head, C):
    """v1's header with component 1's sampling byte 0x22 (C = 3 only)"""
    if C == 1:
        return head
    at = head.index(b"\xff\xc0") + 10              # marker, length, precision, H, W, Nf -> component 1's id
    assert head[at:at + 3] == b"\x01\x11\x00"
    return head[:at + 1] + b"\x22" + head[at + 2:]


def header(H, W, C, quality, restart):
    return _sampled(ref.header(H, W, C, quality, restart), C)


def header_optimal(H, W, C, quality, restart, tables):
    return _sampled(opt.header_optimal(H, W, C, quality, restart, tables), C)


def _shape(a):
    return a.shape[0], a.shape[1], 1 if is_gray(a) else 3


def encode(img, quality=100, restart=8):
    """a whole JFIF file"""
    a = np.asarray(img)
    return header(*_shape(a), quality, restart) + scan(a, quality, restart) + b"\xff\xd9"


def encode_optimal(img, quality=100, restart=8):
    a = np.asarray(img)
    body, tables = scan_optimal(a, quality, restart)
    return header_optimal(*_shape(a), quality, restart, tables) + body + b"\xff\xd9"


def blocks(H, W, C):
    """8 x 8 blocks of an image's scan in 4:2:0 mode"""
    return ((H + 7) // 8) * ((W + 7) // 8) if C == 1 else 6 * ((H + 15) // 16) * ((W + 15) // 16)


def mcus(H, W, C):
    return blocks(H, W, C) // (1 if C == 1 else 6)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def smooth_image(h, w, seed=20261019):
    """seeded smooth RGB: one slow wave per channel with its own phase, sigma 2 noise"""
    rng = np.random.default_rng(seed + 1000 * h + w)
    yy, xx = np.mgrid[:h, :w]
    ph = rng.uniform(0.0, 6.28, 3)
    img = np.stack([128 + 80 * np.sin(xx / 11.0 + ph[c]) * np.cos(yy / 13.0 - ph[c]) + 20 * c for c in range(3)], -1)
    return np.clip(np.rint(img + rng.normal(0.0, 2.0, img.shape)), 0, 255).astype(np.uint8)


LADDER_LEVELS = [16 + 10 * k for k in range(24)]


def ladder_image():
    """32 x 48 RGB, gray-valued: every 8 x 8 block flat, block k in raster order at level 16 + 10 k (24 distinct levels).  A decoder
    returns the levels in place only if the Y blocks of an MCU are written in the order (0,0), (0,1), (1,0), (1,1) and their DC chain
    runs in that order."""
    lv = np.array(LADDER_LEVELS, np.uint8).reshape(4, 6)
    return np.repeat(np.kron(lv, np.ones((8, 8), np.uint8))[:, :, None], 3, axis=2)


def chroma_extreme_images():
    """two 16 x 96 images of six 16 x 16 cells that alternate between opposite corners of the chroma plane: DC differences of size 11
    in table 1 (one chroma block per MCU)"""
    out = {}
    for name, (a, b) in (("16x96 blue/yellow", ((0, 0, 255), (255, 255, 0))), ("16x96 red/cyan", ((255, 0, 0), (0, 255, 255)))):
        img = np.empty((16, 96, 3), np.uint8)
        for k in range(6):
            img[:, 16 * k:16 * (k + 1)] = a if k % 2 == 0 else b
        out[name] = img
    return out


def images():
    """{name: image}: everything the 4:2:0 tests encode"""
    photo = ref.photo_image()
    out = {"37x53 noise": ref.noise_image(), "75x100 photo": photo, "75x100 gray": ref.gray_of(photo)}
    for h, w in ((1, 1), (16, 16), (17, 15), (33, 47), (8, 40)):
        out[f"{h}x{w} smooth"] = smooth_image(h, w)
    out["24x520 noise"] = ref.noise_image(24, 520, 3, seed=20261020)      # 33 MCU columns: two whole 256-column strips and one MCU
    out["32x48 ladder"] = ladder_image()
    out.update(chroma_extreme_images())
    return out


QUALITIES = (100, 95, 75, 1)
RESTARTS = (1, 3, 8, 65535)
