"""The restatement of "JPG-SPEC v1, optimal tables" (tests/jpegopt_np.py) held to what it is there for: its table construction is the
one Pillow's libjpeg runs (every DHT table of Pillow's own optimize=True files, bit for bit), its inputs reach the length limiter, its
tables are prefix codes over exactly the used symbols, its files decode to the standard files' pixels and are shorter, and
gs360/jpegenc.py builds the same header from the device's table bytes."""
import io
from fractions import Fraction

import numpy as np
import pytest

from gs360 import jpegenc

import jpegenc_np as ref
import jpegopt_np as opt

SMALL = opt.small_images()
_SPECKLE = []


def speckle():
    if not _SPECKLE:
        _SPECKLE.append(opt.speckle_image())
    return _SPECKLE[0]


def geometry(a):
    H, W = a.shape[:2]
    return H, W, 1 if a.ndim == 2 else a.shape[2], ((H + 7) // 8) * ((W + 7) // 8)


def split_file(data):
    """a JFIF file -> (everything up to and including SOS, the scan, {(class, id): (BITS, HUFFVAL)}, restart interval)"""
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    p, tables, dri = 2, {}, 0
    while True:
        assert data[p] == 0xFF
        marker, n = data[p + 1], int.from_bytes(data[p + 2:p + 4], "big")
        body = data[p + 4:p + 2 + n]
        p += 2 + n
        if marker == 0xC4:
            q = 0
            while q < len(body):
                bits = list(body[q + 1:q + 17])
                tables[(body[q] >> 4, body[q] & 15)] = (bits, list(body[q + 17:q + 17 + sum(bits)]))
                q += 17 + sum(bits)
        elif marker == 0xDD:
            dri = int.from_bytes(body, "big")
        elif marker == 0xDA:
            return data[:p], data[p:-2], tables, dri


def check_pillow_tables(img, quality, restart):
    Image = pytest.importorskip("PIL.Image")
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=quality, subsampling=0, optimize=True, restart_marker_blocks=restart)
    head, scan, tables, dri = split_file(b.getvalue())
    if dri == 0:
        pytest.skip("this Pillow writes no restart intervals (restart_marker_blocks)")
    assert dri == restart
    H, W, C, n_mcu = geometry(img)
    z = ref.decode_scan(head, scan, n_mcu, C)
    hist = opt.symbol_hist(z, restart)
    assert len(tables) == (2 if C == 1 else 4)
    for k, key in enumerate([(0, 0), (1, 0), (0, 1), (1, 1)][:len(tables)]):
        bits, vals = opt.optimal_table(hist[k])
        assert tables[key] == (bits, vals), (key, quality, restart)


@pytest.mark.parametrize("restart", [1, 8, 1000])
@pytest.mark.parametrize("quality", [100, 95, 75, 10])
@pytest.mark.parametrize("name", list(SMALL))
def test_the_construction_reproduces_pillows_own_tables(name, quality, restart):
    check_pillow_tables(SMALL[name], quality, restart)


def test_the_construction_reproduces_pillows_tables_of_the_speckle_image():
    check_pillow_tables(speckle(), 95, 8)


def test_the_speckle_image_reaches_the_length_limiter():
    """both AC tables of the speckle image at quality 100, Ri 8 have codes longer than 16 bits before limiting (measured: 17 and 19)"""
    hist = opt.symbol_hist(ref.coefficients(speckle(), 100), 8)
    longest = [opt.max_unlimited_length(hist[1]), opt.max_unlimited_length(hist[3])]
    print("unlimited maximum lengths, luma AC / chroma AC:", longest)
    assert min(longest) > 16
    for h in (hist[1], hist[3]):
        bits, vals = opt.optimal_table(h)
        assert sum(bits) == len(vals) == sum(1 for v in h if v)


@pytest.mark.parametrize("name", list(opt.synthetic_histograms()))
def test_synthetic_histograms_give_prefix_codes_over_the_used_symbols(name):
    h = opt.synthetic_histograms()[name]
    bits, vals = opt.optimal_table(h)
    used = [s for s in range(256) if h[s]]
    assert len(bits) == 16 and sum(bits) == len(used)               # (no length above 16: BITS has sixteen entries and holds them all)
    assert sorted(vals) == used and len(set(vals)) == len(vals)
    kraft = sum(Fraction(n, 1 << (i + 1)) for i, n in enumerate(bits))
    assert kraft + Fraction(1, 1 << max(i + 1 for i, n in enumerate(bits) if n)) <= 1     # the all-ones code stays free
    codes = ref.huff_codes((bits, vals))
    assert all(code != (1 << length) - 1 for code, length in codes.values())
    if name.startswith(("fibonacci", "powers")):
        longest = opt.max_unlimited_length(h)
        print("unlimited maximum length:", longest)
        assert longest > (25 if name.startswith("powers") else 16)


def test_an_all_zero_histogram_gives_the_all_zero_table():
    assert opt.optimal_table([0] * 256) == ([0] * 16, [])
    assert opt.table_bytes(opt.optimal_table([0] * 256)) == bytes(272)


def _round_trip(img, quality, restart):
    Image = pytest.importorskip("PIL.Image")
    H, W, C, n_mcu = geometry(img)
    scan, tables = opt.scan_optimal(img, quality, restart)
    head = opt.header_optimal(H, W, C, quality, restart, tables)
    z = ref.coefficients(img, quality).reshape(n_mcu, C, 64)
    assert np.array_equal(ref.decode_scan(head, scan, n_mcu, C), z)
    f_opt, f_std = opt.encode_optimal(img, quality, restart), ref.encode(img, quality, restart)
    assert f_opt == head + scan + b"\xff\xd9"
    a, b = np.asarray(Image.open(io.BytesIO(f_opt))), np.asarray(Image.open(io.BytesIO(f_std)))
    assert a.shape == img.shape and np.array_equal(a, b)            # same coefficients, same decoder
    print(f"{len(f_std)} -> {len(f_opt)} bytes")
    assert len(f_opt) < len(f_std)                                  # checked on these images, not a theorem (pseudo-symbol, limiter)
    # gs360/jpegenc.py builds the same header from the device's table bytes; without them today's header
    dev = b"".join(opt.table_bytes(t) for t in tables)
    assert jpegenc.header(H, W, C, quality, restart, tables=dev) == head
    assert jpegenc.header(H, W, C, quality, restart, tables=None) == jpegenc.header(H, W, C, quality, restart) == ref.header(H, W, C, quality, restart)


@pytest.mark.parametrize("quality,restart", [(100, 8), (95, 1), (75, 8), (10, 1000)])
@pytest.mark.parametrize("name", list(SMALL))
def test_optimal_files_round_trip_match_the_standard_pixels_and_are_shorter(name, quality, restart):
    _round_trip(SMALL[name], quality, restart)


def test_the_speckle_image_round_trips_through_the_length_limiter():
    _round_trip(speckle(), 100, 8)


def test_header_rejects_table_bytes_of_the_wrong_size():
    with pytest.raises(ValueError):
        jpegenc.header(8, 8, 3, 90, 8, tables=bytes(272))
