"""The images the PNG-SPEC v1 tests encode (tests/test_pngenc_cpu.py with the NumPy restatement, tests/test_pngenc_gpu.py on the device):
the smallest shapes that reach each hazard of the encoder, and the two seeded fixtures of the size conditions."""
import numpy as np

CHUNK, SEGMENT = 65536, 512          # PNG-SPEC v1's constants (tests/pngenc_np.py)


def _photo(H, W, C, dtype, seed):
    """smooth fields plus about 1.5 LSB of noise"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    top = 255.0 if dtype == np.uint8 else 65535.0
    planes = []
    for c in range(C):
        f = 0.5 + 0.25 * np.sin(xx / (17.0 + 5 * c) + c) * np.cos(yy / (23.0 - 3 * c)) + 0.2 * np.sin((xx + 2 * yy) / (61.0 + 7 * c))
        planes.append(f * top + rng.normal(0.0, 1.5, size=(H, W)))
    return np.clip(np.rint(np.stack(planes, -1)), 0, top).astype(dtype)


def photo_fixture(dtype):
    """the size condition's photo-like image: 256 x 256 RGB"""
    return _photo(256, 256, 3, dtype, 20261019)


def mask_fixture():
    """the size condition's mask: a filled circle, 0 / 255, one channel"""
    yy, xx = np.ogrid[:512, :512]
    return np.where((yy - 250) ** 2 + (xx - 262) ** 2 <= 200 ** 2, 255, 0).astype(np.uint8)[:, :, None]


def _alternating(n):
    return np.where(np.arange(n) % 2 == 0, 1, 255).astype(np.uint8)


def filters_image():
    """64 gray columns; rows built so that every filter type wins a row (tests/test_pngenc_cpu.py checks which) and row 0 ties
    exactly between None and Up (the row above row 0 is zeros), which the lower type takes"""
    rng = np.random.default_rng(7)
    W = 64
    r0 = _alternating(W)                                              # None (= Up on row 0)
    r1 = ((10 + 3 * np.arange(W)) % 256).astype(np.uint8)             # Sub: a ramp
    r2 = (r1.astype(int) + np.where(np.arange(W) % 2 == 0, 1, -1)).astype(np.uint8)    # Up: the ramp again, +-1
    r3 = rng.integers(0, 256, W).astype(np.uint8)
    r4 = np.zeros(W, np.uint8)                                        # Average: each byte the mean of its left and upper neighbour
    for i in range(W):
        r4[i] = ((int(r4[i - 1]) if i else 0) + int(r3[i])) >> 1
    r5 = np.concatenate([rng.integers(0, 256, W // 2), np.full(W // 2, 77)]).astype(np.uint8)
    r6 = np.concatenate([r5[:W // 2], np.full(W // 2, 200)]).astype(np.uint8)          # Paeth: copies the row above, then runs flat
    return np.stack([r0, r1, r2, r3, r4, r5, r6])[:, :, None]


def runs_image():
    """one gray row whose bytes are 0, 1 or 255, so filter None wins and the filtered stream is the row behind one 0: zero runs of
    exactly 259 (a literal and one match of 258) and of 400 (258, then the rest), a run across the end of segment 2, and runs of four
    and of three equal bytes (a match of 3; two literals where a match would be 2)"""
    parts = [_alternating(9), np.zeros(259, np.uint8), _alternating(30), np.ones(4, np.uint8), _alternating(11)[1:], np.ones(3, np.uint8),
             _alternating(20)[1:]]
    used = 1 + sum(len(p) for p in parts)
    parts += [_alternating(SEGMENT + 40 - used), np.zeros(400, np.uint8), _alternating(31)]
    used = 1 + sum(len(p) for p in parts)
    parts += [_alternating(3 * SEGMENT - 100 - used), np.zeros(150, np.uint8), _alternating(77)]
    return np.concatenate(parts)[None, :, None]


def fibonacci_image():
    """one gray row of 4 179 small-magnitude bytes whose values occur 1, 2, 3, 5 ... 1 597 times, arranged so that no byte stands three
    times in a row (no matches: the histogram is the bytes', and the end-of-block symbol is the Fibonacci series' other 1): every
    Huffman merge takes the tree built so far, so an unlimited code for them is 16 bits deep"""
    fib = [1, 2]
    while len(fib) < 16:
        fib.append(fib[-1] + fib[-2])
    values = [0, 1, 255, 2, 254, 3, 253, 4, 252, 5, 251, 6, 250, 7, 249, 8]            # the most frequent first
    left = dict(zip(values, fib[::-1]))
    data = []
    while len(data) < sum(fib):                                                        # the most frequent value that makes no triple
        v = max((v for v in values if left[v] and data[-2:] != [v, v]), key=lambda v: left[v])
        data.append(v)
        left[v] -= 1
    return np.array(data, np.uint8)[None, :, None]


def shifted_rows_image():
    """gray rows that are one random walk, each 64 above the row before: every row takes Sub and the residuals repeat at the row
    distance"""
    rng = np.random.default_rng(5)
    walk = (100 + np.cumsum(rng.choice([-2, -1, 1, 2], size=120))).astype(np.int64)
    return np.stack([(walk + 64 * y) % 256 for y in range(4)]).astype(np.uint8)[:, :, None]


def cases():
    """{name: H x W x C array}"""
    rng = np.random.default_rng(20261019)
    out = {
        "deg_1x1": np.array([[[9, 200, 31]]], np.uint8),
        "deg_1x300": _photo(1, 300, 1, np.uint8, 1),
        "deg_300x1": _photo(300, 1, 3, np.uint16, 2),
        "filters": filters_image(),
        # 1 + W * bpp = 259 = 7 * 37: the rows drift across the segment seams and one chunk seam (260 rows: 67 340 bytes)
        "seams_coprime": _photo(260, 86, 3, np.uint8, 3),
        # rows of 256 bytes: exactly one chunk, exactly two, one row over one, one row over two
        "chunk_exact": _photo(256, 255, 1, np.uint8, 4),
        "chunk_exact2": _photo(512, 255, 1, np.uint8, 5),
        "chunk_over1": _photo(257, 255, 1, np.uint8, 6),
        "chunk_over2": _photo(513, 255, 1, np.uint8, 7),
        "runs": runs_image(),
        "flat_rgb": np.broadcast_to(np.array([40, 90, 200], np.uint8), (9, 50, 3)).copy(),
        "ramp_rgb": ((np.arange(70)[None, :, None] * np.array([1, 2, 3]) + np.array([5, 60, 17])) % 256).astype(np.uint8).repeat(3, axis=0),
        "repeated_row": np.repeat(_photo(1, 90, 3, np.uint8, 8), 5, axis=0),
        "shifted_rows": shifted_rows_image(),
        "noise": rng.integers(0, 256, size=(70, 67, 1)).astype(np.uint8),
        "zeros": np.zeros((40, 33, 3), np.uint8),
        "fibonacci": fibonacci_image(),
    }
    for C in (1, 3, 4):
        for dtype, tag in ((np.uint8, "u8"), (np.uint16, "u16")):
            out[f"c{C}_{tag}"] = _photo(37, 53, C, dtype, 10 * C + len(tag))
    return out
