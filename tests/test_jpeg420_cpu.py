""""JPG-SPEC v1, 4:2:0" without a GPU: the NumPy restatement (tests/jpeg420_np.py) against Pillow's decoder, Pillow's own
`subsampling=2` files and answers worked out by hand, and the header gs360/jpegenc.py builds for the mode."""
import functools
import io

import numpy as np
import pytest

from gs360 import jpegenc

import jpeg420_np as j420
import jpegenc_np as ref
import jpegopt_np as opt

IMAGES = j420.images()
NAMES = list(IMAGES)


def segments(data):
    """{marker: [payload, ...]} of a JFIF file's header segments, up to and including SOS"""
    out, p = {}, 2
    assert data[:2] == b"\xff\xd8"
    while True:
        assert data[p] == 0xFF
        marker, n = data[p + 1], int.from_bytes(data[p + 2:p + 4], "big")
        out.setdefault(marker, []).append(data[p + 4:p + 2 + n])
        p += 2 + n
        if marker == 0xDA:
            return out


def quant_payloads(payloads):
    out = {}
    for pl in payloads:
        for p in range(0, len(pl), 65):
            out[pl[p]] = bytes(pl[p + 1:p + 65])
    return out


def open_file(data):
    Image = pytest.importorskip("PIL.Image")
    return Image.open(io.BytesIO(data))


def decode(data):
    return np.asarray(open_file(data))


def pillow_file(a, quality, **kw):
    Image = pytest.importorskip("PIL.Image")
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", quality=quality, subsampling=2, **kw)
    return b.getvalue()


def psnr(a, b):
    return 10.0 * np.log10(255.0 ** 2 / max(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2), 1e-12))


@functools.lru_cache(maxsize=None)
def coefficients(name, quality):
    return j420.coefficients(IMAGES[name], quality)


def encode(name, quality, restart):
    a = IMAGES[name]
    if j420.is_gray(a):
        return j420.encode(a, quality, restart)
    return (j420.header(a.shape[0], a.shape[1], 3, quality, restart) + j420.scan_from_coefficients(coefficients(name, quality), restart)
            + b"\xff\xd9")


def test_the_inputs_are_the_ones_the_spec_names():
    assert [IMAGES[n].shape for n in NAMES] == [(37, 53, 3), (75, 100, 3), (75, 100), (1, 1, 3), (16, 16, 3), (17, 15, 3), (33, 47, 3),
                                                (8, 40, 3), (24, 520, 3), (32, 48, 3), (16, 96, 3), (16, 96, 3)]
    lad = IMAGES["32x48 ladder"]
    assert len(set(j420.LADDER_LEVELS)) == 24 and max(j420.LADDER_LEVELS) == 246
    for k, level in enumerate(j420.LADDER_LEVELS):
        assert (lad[8 * (k // 6):8 * (k // 6) + 8, 8 * (k % 6):8 * (k % 6) + 8] == level).all()
    assert coefficients("24x520 noise", 100).shape == (2, 33, 6, 64)              # two whole 256-column strips and one MCU
    for name in ("16x96 blue/yellow", "16x96 red/cyan"):                         # DC differences of size 11 in table 1
        h = j420.symbol_hist(coefficients(name, 100), 8)
        assert h[2][11] >= 2, name


@pytest.mark.parametrize("quality", j420.QUALITIES)
@pytest.mark.parametrize("name", NAMES)
def test_pillow_decodes_every_image_at_every_restart_interval(name, quality):
    from PIL import JpegImagePlugin
    a = IMAGES[name]
    for restart in j420.RESTARTS:
        im = open_file(encode(name, quality, restart))
        got = np.asarray(im)
        assert got.shape == a.shape, restart
        if a.ndim == 3:
            assert JpegImagePlugin.get_sampling(im) == 2, restart
        if restart != j420.RESTARTS[0]:
            assert np.array_equal(got, first), restart                            # the interval changes the stream, not the picture
        first = got


def test_gray_files_are_v1s_bytes():
    g = IMAGES["75x100 gray"]
    for quality, restart in ((100, 8), (75, 3), (1, 65535)):
        assert j420.encode(g, quality, restart) == ref.encode(g, quality, restart)
        assert j420.encode_optimal(g, quality, restart) == opt.encode_optimal(g, quality, restart)
        assert j420.header(75, 100, 1, quality, restart) == ref.header(75, 100, 1, quality, restart)


@pytest.mark.parametrize("restart", [1, 8])
def test_ladder_levels_come_back_in_place(restart):
    """Pillow's decoder at quality 100: every 8 x 8 block's mean within 1 of its level.  The 24 levels are distinct and 10 apart, so
    a wrong Y block order inside the MCU or a DC chain in another order moves a level by 10 or more."""
    got = decode(encode("32x48 ladder", 100, restart)).astype(np.float64)
    for k, level in enumerate(j420.LADDER_LEVELS):
        blk = got[8 * (k // 6):8 * (k // 6) + 8, 8 * (k % 6):8 * (k % 6) + 8]
        assert abs(blk.mean() - level) <= 1.0, (k, blk.mean(), level)


def test_downsample_known_answers():
    """(a + b + c + d + bias) >> 2, bias 1 at even and 2 at odd output columns: cell sums 1, 2, 3 give 0, 0, 1 at an even column
    ((1 + 1) >> 2, (2 + 1) >> 2, (3 + 1) >> 2) and 0, 1, 1 at an odd one ((1 + 2) >> 2, (2 + 2) >> 2, (3 + 2) >> 2)"""
    cells = {1: [[1, 0], [0, 0]], 2: [[0, 1], [1, 0]], 3: [[1, 1], [0, 1]]}
    for s, even, odd in ((1, 0, 0), (2, 0, 1), (3, 1, 1)):
        plane = np.hstack([np.array(cells[s]), np.array(cells[s])])                # 2 x 4: the same cell at columns 0 and 1
        assert j420.downsample(plane).tolist() == [[even, odd]], s
    big = np.array([[255, 255, 255, 255], [255, 255, 255, 254]])
    assert j420.downsample(big).tolist() == [[255, 255]]                          # (1020 + 1) >> 2, (1019 + 2) >> 2
    assert j420.downsample(np.arange(32).reshape(4, 8)).shape == (2, 4)


def test_planes_pad_to_sixteen_before_the_downsample():
    a = IMAGES["17x15 smooth"]
    Y, Cb, Cr = j420.planes(a)
    assert Y.shape == (32, 16) and Cb.shape == Cr.shape == (16, 8)
    full = ref.planes(np.pad(a, ((0, 15), (0, 1), (0, 0)), mode="edge"))
    assert np.array_equal(Y, full[0])
    assert np.array_equal(Cb + 128, j420.downsample(full[1] + 128)) and np.array_equal(Cr + 128, j420.downsample(full[2] + 128))
    assert (Cb[9:] == Cb[8]).all() and (Y[17:] == Y[16]).all()                    # rows below the image repeat its last row


def test_header_equals_the_restatements_and_pillows_quantisers():
    for C in (1, 3):
        a = ref.noise_image(16, 16, C)
        for quality, restart in ((100, 8), (95, 1), (75, 3), (1, 65535)):
            h = jpegenc.header(37, 53, C, quality, restart, subsampling="4:2:0")
            assert h == j420.header(37, 53, C, quality, restart)
            sof = segments(h)[0xC0][0]
            assert [sof[6 + 3 * c + 1] for c in range(C)] == ([0x22, 0x11, 0x11] if C == 3 else [0x11])
            theirs = segments(pillow_file(a, quality))
            assert quant_payloads(segments(h)[0xDB]) == quant_payloads(theirs[0xDB])
            assert jpegenc.header(37, 53, C, quality, restart, subsampling="4:4:4") == jpegenc.header(37, 53, C, quality, restart) \
                == ref.header(37, 53, C, quality, restart)
    scan, tabs = j420.scan_optimal(IMAGES["37x53 noise"], 95, 8)
    raw = b"".join(opt.table_bytes(t) for t in tabs)
    assert jpegenc.header(37, 53, 3, 95, 8, raw, subsampling="4:2:0") == j420.header_optimal(37, 53, 3, 95, 8, tabs)
    with pytest.raises(ValueError):
        jpegenc.header(8, 8, 3, 90, 8, subsampling="4:2:2")


@pytest.mark.parametrize("quality", j420.QUALITIES)
@pytest.mark.parametrize("name", NAMES)
def test_fidelity_is_within_half_a_db_of_pillows_420_encoder(name, quality):
    """PSNR against the source of our decoded file, minus the same for Pillow's `subsampling=2` file at that quality: at least -0.5 dB
    (the bound of the 4:4:4 test).  The measured table is in DESIGN.md section 11; the worst deficit there is -0.26 dB (17x15 smooth,
    quality 95).  Noise is here to show nothing breaks: about 12.8 dB for both encoders."""
    a = IMAGES[name]
    ours = psnr(decode(encode(name, quality, 8)), a)
    theirs = psnr(decode(pillow_file(a, quality)), a)
    print(f"{name} quality {quality}: ours {ours:.2f} dB, Pillow {theirs:.2f} dB, difference {ours - theirs:+.2f} dB")
    assert ours - theirs >= -0.5


class _Tally(dict):
    """a code table that counts the symbols the coder asks it for"""

    def __init__(self):
        super().__init__()
        self.count = [0] * 256

    def __getitem__(self, symbol):
        self.count[symbol] += 1
        return (0, 1)


@pytest.mark.parametrize("name", ["37x53 noise", "75x100 photo", "24x520 noise", "75x100 gray", "32x48 ladder", "16x96 red/cyan"])
def test_optimal_tables_decode_and_count_the_symbols_the_coder_emits(name):
    a = IMAGES[name]
    for quality, restart in ((100, 8), (75, 3), (95, 65535)):
        data = j420.encode_optimal(a, quality, restart)
        got = decode(data)
        assert got.shape == a.shape and np.array_equal(got, decode(encode(name, quality, restart)))   # other codes, the same coefficients
        assert len(data) <= len(encode(name, quality, restart))
        if j420.is_gray(a):
            continue
        z = coefficients(name, quality).reshape(-1, 6, 64)
        tally = [_Tally() for _ in range(4)]                                      # the coder's own walk, counted at its table lookups
        w, pred = ref.BitWriter(), [0, 0, 0]
        for m in range(len(z)):
            if m % restart == 0:
                pred = [0, 0, 0]
            for i, c in enumerate(j420.COMP_OF):
                t = 2 if c else 0
                ref.encode_block(w, z[m, i], pred[c], tally[t], tally[t + 1])
                pred[c] = int(z[m, i, 0])
        hist = j420.symbol_hist(z, restart)
        assert [t.count for t in tally] == hist
        _scan, tables = j420.scan_optimal(a, quality, restart)
        for h, (bits, vals) in zip(hist, tables):
            assert sorted(vals) == [s for s in range(256) if h[s]] and sum(bits) == len(vals)
        assert sum(hist[0]) == 4 * len(z) and sum(hist[2]) == 2 * len(z)          # one DC symbol per block: table 0 Y, table 1 Cb and Cr
