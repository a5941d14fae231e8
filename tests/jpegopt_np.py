""""JPG-SPEC v1, optimal tables"  restated in plain Python on top of tests/jpegenc_np.py: the symbols a scan emits,
T.81 Annex K.2 as libjpeg's jpeg_gen_optimal_table runs it (others[] chain and all), and the scan, header and file they give.
Independent of gs360/jpegenc.py and of the HIP kernels: the tests compare both against this, and this against Pillow's own files."""
import numpy as np

import jpegenc_np as ref

TABLE_BYTES = 272             # 16 BITS + up to 256 HUFFVAL, zero padded (GS360_JPEG_TABLE_BYTES)


def symbol_hist(z, restart):
    """coefficients [blocks_y][blocks_x][C][64] or [n_mcu][C][64] -> [DC0, AC0, DC1, AC1], 256 counts each: the symbols
    jpegenc_np.encode_block emits, with the DC prediction reset at every restart interval.  DC1 and AC1 stay zero for C = 1."""
    z = np.asarray(z)
    mcus = z.reshape(-1, z.shape[-2], 64)
    C = mcus.shape[1]
    hist = [[0] * 256 for _ in range(4)]
    pred = [0] * C
    for m in range(len(mcus)):
        if m % restart == 0:
            pred = [0] * C
        for c in range(C):
            t = 2 if c else 0
            blk = [int(v) for v in mcus[m, c]]
            hist[t][abs(blk[0] - pred[c]).bit_length()] += 1
            pred[c] = blk[0]
            run = 0
            for v in blk[1:]:
                if v == 0:
                    run += 1
                    continue
                while run > 15:
                    hist[t + 1][0xF0] += 1
                    run -= 16
                hist[t + 1][(run << 4) | abs(v).bit_length()] += 1
                run = 0
            if run:
                hist[t + 1][0x00] += 1
    return hist


def code_lengths(freq):
    """the merge loop of jpeg_gen_optimal_table -> 257 unlimited code lengths (entry 256: the pseudo-symbol)"""
    f = [int(v) for v in freq] + [1]
    assert len(f) == 257 and min(f) >= 0 and sum(f) <= 10 ** 9
    codesize, others = [0] * 257, [-1] * 257
    while True:
        c1, v = -1, 10 ** 9
        for i in range(257):
            if f[i] and f[i] <= v:                # <=: ties go to the largest index
                v, c1 = f[i], i
        c2, v = -1, 10 ** 9
        for i in range(257):
            if f[i] and f[i] <= v and i != c1:
                v, c2 = f[i], i
        if c2 < 0:
            return codesize
        f[c1] += f[c2]
        f[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1


def optimal_table(freq):
    """256 symbol counts -> (BITS[1..16], HUFFVAL); ([0] * 16, []) for an all-zero histogram"""
    if not any(freq):
        return [0] * 16, []
    codesize = code_lengths(freq)
    bits = [0] * 65
    for n in codesize:
        if n:
            bits[n] += 1
    for i in range(64, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                                  # the pseudo-symbol's code, the all-ones one
    vals = [s for n in range(1, 65) for s in range(256) if codesize[s] == n]
    assert sum(bits[1:17]) == len(vals) and not any(bits[17:])
    return bits[1:17], vals


def table_bytes(table):
    """(BITS, HUFFVAL) -> the 272 bytes the device returns for it"""
    bits, vals = table
    return bytes(bits) + bytes(vals) + bytes(TABLE_BYTES - 16 - len(vals))


def scan_from_coefficients_optimal(z, restart=8):
    """-> (scan, [DC0, AC0, DC1, AC1] as (BITS, HUFFVAL)); jpegenc_np.scan_from_coefficients with the image's own tables"""
    by, bx, C, _ = z.shape
    mcus = z.reshape(by * bx, C, 64)
    tables = [optimal_table(h) for h in symbol_hist(mcus, restart)]
    codes = [ref.huff_codes(t) for t in tables]
    out = bytearray()
    n = len(mcus)
    n_int = (n + restart - 1) // restart
    for k in range(n_int):
        w = ref.BitWriter()
        pred = [0] * C
        for m in range(k * restart, min(n, (k + 1) * restart)):
            for c in range(C):
                t = 2 if c else 0
                ref.encode_block(w, mcus[m, c], pred[c], codes[t], codes[t + 1])
                pred[c] = int(mcus[m, c, 0])
        w.pad()
        out += w.out
        if k + 1 < n_int:
            out += bytes([0xFF, 0xD0 + (k & 7)])
    return bytes(out), tables


def scan_optimal(img, quality=100, restart=8):
    a = np.asarray(img)
    ref._check_args(1 if a.ndim == 2 else a.shape[2], quality, restart)
    return scan_from_coefficients_optimal(ref.coefficients(a, quality), restart)


def header_optimal(H, W, C, quality, restart, tables):
    """jpegenc_np.header with the DHT payloads taken from `tables` ([DC0, AC0, DC1, AC1]; the first two for C = 1)"""
    std = ref.header(H, W, C, quality, restart)
    out, p, k = bytearray(std[:2]), 2, 0
    while p < len(std):
        n = int.from_bytes(std[p + 2:p + 4], "big")
        if std[p + 1] == 0xC4:
            bits, vals = tables[k]
            out += ref._seg(0xC4, bytes([std[p + 4]]) + bytes(bits) + bytes(vals))
            k += 1
        else:
            out += std[p:p + 2 + n]
        p += 2 + n
    assert k == (2 if C == 1 else 4)
    return bytes(out)


def encode_optimal(img, quality=100, restart=8):
    """a whole JFIF file"""
    a = np.asarray(img)
    H, W = a.shape[:2]
    C = 1 if a.ndim == 2 else a.shape[2]
    scan, tables = scan_optimal(a, quality, restart)
    return header_optimal(H, W, C, quality, restart, tables) + scan + b"\xff\xd9"


def max_unlimited_length(freq):
    return max(code_lengths(freq)[:256])


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def speckle_image():
    """512 x 512 RGB: smooth waves, a coarse checker, sigma 1.5 noise and sparse bright speckles.  At quality 100 its rare AC symbols
    sit next to very common ones: both AC tables need more than 16 bits before limiting."""
    H = W = 512
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[:H, :W]
    img = np.stack([128 + 70 * np.sin(xx / 23 + c) * np.cos(yy / 17 - c) + 40 * (((xx // 64) + (yy // 48)) % 2) for c in range(3)], -1)
    img = img + rng.normal(0, 1.5, img.shape)
    img = img + (rng.random(img.shape) < 0.002) * 120
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def small_images():
    """the five small images of the CPU tests: noise, photo, gray, checker, flat"""
    photo = ref.photo_image()
    return {"37x53 noise": ref.noise_image(), "75x100 photo": photo, "33x41 gray": ref.gray_of(photo)[:33, :41],
            "24x40 checker": ref.checker_image(), "9x17 flat": np.full((9, 17, 3), (255, 0, 128), np.uint8)}


def _fib(n):
    a, b, out = 1, 1, []
    for _ in range(n):
        out.append(a)
        a, b = b, a + b
    return out


def synthetic_histograms():
    """{name: 256 counts} that no small image produces"""
    def put(pairs):
        h = [0] * 256
        for s, n in pairs:
            h[s] = n
        return h
    return {
        "fibonacci over 40": put(zip(range(3, 43), _fib(40))),                 # lengths far above 16 before limiting
        "powers of two descending": put((200 + k, 1 << (28 - k)) for k in range(29)),      # a chain: one more bit per symbol
        "256 ascending": [s + 1 for s in range(256)],
        "one symbol": put([(0x21, 7)]),
        "two symbols": put([(0x00, 5), (0xF0, 5)]),
        "all 256 equal": [3] * 256,
        "162 ones beside 1e8": put([(s, 1) for s in range(1, 163)] + [(0, 10 ** 8)]),
    }
