"""The images the PNG-SPEC v1 tests encode (tests/test_pngenc_cpu.py with the NumPy restatement, tests/test_pngenc_gpu.py on the device):
the smallest shapes that reach each hazard of the encoder, the two seeded fixtures of the size conditions, and (alphabet_cases(), for
tests/test_pngenc_alphabet_gpu.py) the images that reach every match length, both ends of every distance symbol, both sides of the
32 768 bound and the largest sides."""
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


# ---- the length and distance alphabets, the 32 768 bound and the largest sides (tests/test_pngenc_alphabet_gpu.py) ---------------------
# Each function below has its own seeded generators; cases() and the two size-condition fixtures above do not depend on them.
def lengths_image():
    """one gray row whose bytes are 0, 1 or 255 (filter None wins, as in runs_image): zero runs of every length 4..259 once, shuffled,
    between alternating stretches of 2..5 bytes, none across the end of a 512-byte segment of the filtered stream.  Each run is a
    literal and one distance-1 match, so the matches are every length 3..258 once.  A run that would cross a segment's end gives way
    to the first one left that fits; where none fits the stretch runs on into the next segment.  One chunk."""
    rng = np.random.default_rng(20261101)
    left = [int(v) for v in rng.permutation(np.arange(4, 260))]
    parts, pos = [_alternating(7)], 1 + 7                                              # pos: the filtered stream's (the type byte leads)
    while left:
        gap = int(rng.integers(2, 6))
        room = SEGMENT - (pos + gap) % SEGMENT
        fits = [n for n in left if n <= room]
        if not fits:
            gap += room
        run = fits[0] if fits else left[0]
        left.remove(run)
        parts += [_alternating(gap), np.zeros(run, np.uint8)]
        pos += gap + run
    parts.append(_alternating(9))
    row = np.concatenate(parts)
    assert 1 + len(row) <= CHUNK
    return row[None, :, None]


def alphabet_distances():
    """the first and last distance of each of RFC 1951's 30 distance symbols, without distance 1: 55 distances"""
    firsts = [1, 2, 3, 4] + [(2 + h) * (1 << e) + 1 for e in range(1, 14) for h in (0, 1)]
    lasts = firsts[1:] + [32769]
    return sorted({d for f, l in zip(firsts, lasts) for d in (f, l - 1)} - {1})


def walk_image(H, W, seed):
    """gray 8-bit rows that are one random walk of steps +-1 and +-2, each 64 above the row before (shifted_rows_image's trick): every
    row takes Sub and the residuals repeat at the row distance 1 + W"""
    rng = np.random.default_rng(seed)
    walk = (100 + np.cumsum(rng.choice([-2, -1, 1, 2], size=W))).astype(np.int64)
    return np.stack([(walk + 64 * y) % 256 for y in range(H)]).astype(np.uint8)[:, :, None]


def walk_image_rgba16(H, W, seed):
    """the same for RGBA 16-bit: the four samples of a pixel are the walk's value, and every BYTE of a row is 64 above the row before's,
    so no carry disturbs the repeat.  A pixel's Sub residuals are (0 or +-1, step) four times: nothing repeats at distance 1, equal
    steps repeat at distance 8 = bpp, the rows at 1 + 8 W."""
    rng = np.random.default_rng(seed)
    walk = (1000 + np.cumsum(rng.choice([-2, -1, 1, 2], size=W))).astype(np.int64)
    rows = []
    for y in range(H):
        hi, lo = ((walk >> 8) + 64 * y) % 256, (walk + 64 * y) % 256
        rows.append(np.repeat(((hi << 8) | lo)[:, None], 4, axis=1))
    return np.stack(rows).astype(np.uint16)


def distance_cases():
    """{name: 3 x (d - 1) x 1 walk image} for every distance d >= 5 of alphabet_distances(): the row distance is d.  (2, 3 and 4 are
    cases()'s bpp candidates: rows that short hold no match.)  In call order: ascending, but the three images of more than one chunk
    (d = 24 576, 24 577, 32 768) stand second in the first three launch batches of 16, so the chunks of later jobs and batches lie
    behind theirs.  d = 32 768 is the last distance allowed; its third row is chunk 1 from position 0 to 32 767, every source of a
    row-distance match in front of the chunk."""
    ds = [d for d in alphabet_distances() if d >= 5]
    order = ds[:-3]
    for at, d in zip((1, 17, 33), ds[-3:]):
        order.insert(at, d)
    return {f"dist_{d}": walk_image(3, d - 1, 20261100 + d) for d in order}


def bound_cases():
    """the row candidate on both sides of 32 768, 3 rows each: 32 769 (dropped) and the last ones kept, for bpp = 1 and 8"""
    return {
        "bound_gray_32769": walk_image(3, 32768, 20261201),
        "bound_rgba16_32769": walk_image_rgba16(3, 4096, 20261202),
        "bound_rgba16_32761": walk_image_rgba16(3, 4095, 20261203),
        "bound_gray_32768": walk_image(3, 32767, 20261100 + 32768),                    # distance_cases()'s dist_32768
    }


def side_cases():
    """the largest sides: rows of 524 280 bytes (each across 8 chunks, 16 chunks in all; small values, nine pixels in ten zero) and
    65 535 rows of one byte (a walk, so that Up takes most rows and None some)"""
    rng = np.random.default_rng(20261301)
    wide = (rng.integers(0, 4, size=(2, 65535, 4)) * (rng.random((2, 65535, 1)) < 0.1)).astype(np.uint16)
    rng = np.random.default_rng(20261302)
    tall = ((np.cumsum(rng.integers(-3, 4, size=65535)) + 5) % 256).astype(np.uint8)[:, None, None]
    return {"side_wide_u16": wide, "side_tall_u8": tall}


def alphabet_cases():
    """{name: image} of all of the above"""
    out = {"lengths": lengths_image()}
    out.update(distance_cases())
    out.update(bound_cases())
    out.update(side_cases())
    return out


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
