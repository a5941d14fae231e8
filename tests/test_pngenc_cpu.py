"""PNG-SPEC v1 without a GPU: the NumPy restatement (tests/pngenc_np.py) against Pillow, the package's 16-bit reader and zlib, the cases
(tests/pngenc_cases.py) against the hazards they are there for, the size conditions, and gs360/pngenc.py's host half."""
import io
import zlib

import numpy as np
import pytest
from PIL import Image

from gs360 import imageio, pngenc

import pngenc_cases as cases
import pngenc_np as ref

IMAGES = cases.cases()
_FILES = {}


def png_of(name):
    if name not in _FILES:
        _FILES[name] = ref.encode(IMAGES[name])
    return _FILES[name]


def symbols_of(img):
    """[the symbol list of every chunk]"""
    rows, bpp, _C, _depth = ref.image_bytes(img)
    stream = ref.filter_rows(rows, bpp)[0].reshape(-1)
    dists = ref.candidate_distances(rows.shape[1] // bpp, bpp)
    return [ref.parse_chunk(stream[c0:c0 + ref.CHUNK], dists) for c0 in range(0, len(stream), ref.CHUNK)]


@pytest.mark.parametrize("name", list(IMAGES))
def test_the_restatements_file_decodes_to_the_pixels(name):
    img, png = IMAGES[name], png_of(name)
    if img.dtype == np.uint8:
        with Image.open(io.BytesIO(png)) as im:
            assert im.mode == {1: "L", 3: "RGB", 4: "RGBA"}[img.shape[2]]
            got = np.asarray(im)
    else:
        got = imageio._png_read(png)
    assert got.dtype == img.dtype and np.array_equal(got.reshape(img.shape), img)


@pytest.mark.parametrize("name", list(IMAGES))
def test_zlib_inflates_the_idat_payload_to_the_filtered_stream(name):
    """zlib checks the block syntax and the Adler-32 on its own"""
    assert zlib.decompress(ref.idat_payload(png_of(name))) == ref.filtered_stream(IMAGES[name]).tobytes()


def test_constants_agree_with_the_package():
    assert ref.CHUNK == cases.CHUNK == pngenc.CHUNK and ref.SEGMENT == cases.SEGMENT
    assert ref.SIGNATURE == pngenc.SIGNATURE and ref.ZLIB_HEADER == pngenc.ZLIB_HEADER


def test_every_filter_type_wins_a_row_and_a_tie_goes_to_the_lower_type():
    rows, bpp, _C, _depth = ref.image_bytes(IMAGES["filters"])
    _stream, types, cost = ref.filter_rows(rows, bpp)
    assert sorted(set(types.tolist())) == [0, 1, 2, 3, 4]
    assert cost[0, 0] == cost[2, 0] == cost[:, 0].min() and types[0] == 0         # row 0: None and Up tie exactly, None takes it
    for y, t in enumerate(types):                                                  # and some rows are won outright
        assert cost[t, y] == cost[:, y].min()
    assert sum(int((cost[:, y] == cost[:, y].min()).sum() == 1) for y in range(len(types))) >= 3


def test_the_cases_reach_their_hazards():
    flat = {name: [s for chunk in symbols_of(img) for s in chunk] for name, img in IMAGES.items()}
    lengths = {name: [s[0] for s in syms if len(s) == 2] for name, syms in flat.items()}
    runs = lengths["runs"]
    assert runs.count(258) == 2 and 3 in runs and min(runs) == 3                   # exactly 258; 258 and the rest; a match of three
    assert 400 - 1 - 258 in runs
    # the run across the end of segment 2: a match that stops at the seam, the next segment starts with a match
    chunk = symbols_of(IMAGES["runs"])[0]
    ends, q = set(), 0
    for s in chunk:
        q += s[0] if len(s) == 2 else 1
        if len(s) == 2:
            ends.add(q)
    assert 3 * ref.SEGMENT in ends
    used = {name: {s[1] for s in syms if len(s) == 2} for name, syms in flat.items()}
    assert used["ramp_rgb"] >= {3} and used["flat_rgb"] >= {1}                     # previous pixel; run
    assert 1 + 120 in used["shifted_rows"]                                         # row above
    assert used["noise"] == set()                                                  # no match: the distance alphabet is unused
    assert len({s[0] for s in flat["noise"]}) == 256                               # all 256 literals
    assert {s for s in flat["zeros"] if len(s) == 1} == {(0,)} and used["zeros"] == {1}
    rows, bpp, _C, _depth = ref.image_bytes(IMAGES["seams_coprime"])
    assert np.gcd(1 + rows.shape[1], ref.SEGMENT) == 1 and rows.shape[0] * (1 + rows.shape[1]) > ref.CHUNK
    sizes = {n: IMAGES[n].shape[0] * (1 + IMAGES[n].shape[1]) for n in ("chunk_exact", "chunk_exact2", "chunk_over1", "chunk_over2")}
    assert sizes == {"chunk_exact": ref.CHUNK, "chunk_exact2": 2 * ref.CHUNK, "chunk_over1": ref.CHUNK + 256, "chunk_over2": 2 * ref.CHUNK + 256}


# ---- the length and distance alphabets, the 32 768 bound, the largest sides -----------------------------------------------------------
ALPHABET = cases.alphabet_cases()
_RESTATED, _SYMBOLS = {}, {}


def restated(name):
    """-> (deflate bytes, [(adler a, adler b)] per chunk, the whole file) of an alphabet fixture by the restatement, computed once for
    the CPU tests here and the device tests of tests/test_pngenc_alphabet_gpu.py"""
    if name not in _RESTATED:
        img = ALPHABET[name]
        rows, _bpp, C, depth = ref.image_bytes(img)
        deflated, parts = ref.deflate(img)
        png = ref.assemble(img.shape[0], img.shape[1], C, depth, deflated, ref.adler_combine(parts))
        _RESTATED[name] = (deflated, [p[:2] for p in parts], png)
    return _RESTATED[name]


def alphabet_symbols(name):
    if name not in _SYMBOLS:
        _SYMBOLS[name] = symbols_of(ALPHABET[name])
    return _SYMBOLS[name]


def matches_of(chunks):
    return [s for chunk in chunks for s in chunk if len(s) == 2]


def decode_png(png, img):
    """a PNG file -> its pixels in img's shape: Pillow for 8 bits, the package's reader for 16"""
    if img.dtype == np.uint8:
        with Image.open(io.BytesIO(png)) as im:
            assert im.mode == {1: "L", 3: "RGB", 4: "RGBA"}[img.shape[2]]
            got = np.asarray(im)
    else:
        got = imageio._png_read(png)
    assert got.dtype == img.dtype
    return got.reshape(img.shape)


@pytest.mark.parametrize("name", list(ALPHABET))
def test_an_alphabet_fixtures_file_inflates_and_decodes_to_the_pixels(name):
    """zlib and the decoders know RFC 1951's tables on their own: this is what proves the restatement's rows for the symbols that no
    fixture reached before, independently of the kernels"""
    img, png = ALPHABET[name], restated(name)[2]
    assert zlib.decompress(ref.idat_payload(png)) == ref.filtered_stream(img).tobytes()
    assert np.array_equal(decode_png(png, img), img)


def test_the_length_fixture_reaches_every_length():
    (chunk,) = alphabet_symbols("lengths")
    found = matches_of([chunk])
    assert sorted(s[0] for s in found) == list(range(3, 259)) and {s[1] for s in found} == {1}      # every length once, as runs
    coded = {ref._length_symbol(s[0]) for s in found}
    assert {c[0] for c in coded} == set(range(257, 286))
    assert len(coded) == 256 and sum(1 << e for e in ref._LEN_EXTRA) == 257       # every extra value of each symbol but 284's 31st,
    assert (284, 5, 31) not in coded and (285, 0, 0) in coded                      # which is length 258: symbol 285


def test_the_distance_fixtures_reach_both_ends_of_every_distance_symbol():
    listed = cases.alphabet_distances()
    ends = {d for k in range(30) for d in (ref._DIST_BASE[k], (ref._DIST_BASE + [32769])[k + 1] - 1)}
    assert len(listed) == 55 and set(listed) == ends - {1}
    used = set()
    for d in listed[3:]:
        img = ALPHABET[f"dist_{d}"]
        assert img.shape == (3, d - 1, 1) and d in {s[1] for s in matches_of(alphabet_symbols(f"dist_{d}"))}, d
        used.add(d)
    # 2, 3 and 4 (rows too short for a match): the bpp candidates of cases()
    old = {s[1] for img in IMAGES.values() for s in matches_of(symbols_of(img))}
    assert listed[:3] == [2, 3, 4] and old >= {1, 2, 3, 4}
    used |= {1, 2, 3, 4}
    assert {ref._distance_symbol(d)[0] for d in used} == set(range(30))
    assert {ref._distance_symbol(d) for d in used} >= {(k, ref._DIST_EXTRA[k], v) for k in range(30) for v in (0, (1 << ref._DIST_EXTRA[k]) - 1)}
    # the images of more than one chunk stand in front of later jobs and later launch batches of 16
    names = list(cases.distance_cases())
    multi = [i for i, n in enumerate(names) if pngenc.n_chunks(*ALPHABET[n].shape, 1) > 1]
    assert len(names) == 52 and multi == [1, 17, 33] and [pngenc.n_chunks(*ALPHABET[names[i]].shape, 1) for i in multi] == [2, 2, 2]


def test_the_widest_length_and_distance_fields_meet_in_one_match():
    """5 length-extra bits with 13 distance-extra bits, both non-zero: the emit kernel's widest shifts; and the largest extra value a
    distance has, 8191"""
    wide = [(ref._length_symbol(s[0]), ref._distance_symbol(s[1])) for d in (24576, 24577, 32768) for s in matches_of(alphabet_symbols(f"dist_{d}"))]
    assert any(l[1] == 5 and l[2] and e[1] == 13 and e[2] for l, e in wide)
    assert any(l[1] == 5 and l[2] and e == (29, 13, 8191) for l, e in wide) and any(l[1] == 5 and l[2] and e == (28, 13, 8191) for l, e in wide)


def test_the_row_candidate_on_both_sides_of_32768():
    used = {name: [{s[1] for s in chunk if len(s) == 2} for chunk in alphabet_symbols(name)] for name in cases.bound_cases()}
    assert all(len(chunks) == 2 for chunks in used.values())
    assert ALPHABET["bound_gray_32769"].shape == (3, 32768, 1) and used["bound_gray_32769"] == [{1}, {1}]          # 32 769: dropped
    assert ALPHABET["bound_rgba16_32769"].shape == (3, 4096, 4) and used["bound_rgba16_32769"] == [{8}, {8}]       # only bpp is used
    assert ALPHABET["bound_rgba16_32761"].shape == (3, 4095, 4) and 32761 in used["bound_rgba16_32761"][0]         # kept and used
    assert ALPHABET["bound_gray_32768"].shape == (3, 32767, 1) and 32768 in used["bound_gray_32768"][0]            # the last one allowed
    assert np.array_equal(ALPHABET["bound_gray_32768"], ALPHABET["dist_32768"])
    # the third row of the d = 32 768 image is chunk 1 from its first byte on, every position below the distance: a source in front
    # of the chunk, so no row-distance match (the bytes do repeat there: chunk 0 holds such matches)
    stream = ref.filtered_stream(ALPHABET["dist_32768"])
    assert len(stream) == 3 * 32768 and np.array_equal(stream[65536 + 2:], stream[32768 + 2:65536])
    assert 32768 not in used["bound_gray_32768"][1] and used["bound_gray_32768"][1] == {1}
    assert 32761 not in used["bound_rgba16_32761"][1]


def test_the_largest_sides():
    wide, tall = ALPHABET["side_wide_u16"], ALPHABET["side_tall_u8"]
    assert wide.shape == (2, 65535, 4) and wide.dtype == np.uint16 and tall.shape == (65535, 1, 1) and tall.dtype == np.uint8
    assert pngenc.filtered_bytes(2, 65535, 4, 2) == 2 * 524281 and pngenc.n_chunks(2, 65535, 4, 2) == 16 == len(alphabet_symbols("side_wide_u16"))
    assert 524281 > 7 * ref.CHUNK                                                  # a row lies across 8 chunks
    assert pngenc.n_chunks(65535, 1, 1, 1) == 2 == len(alphabet_symbols("side_tall_u8"))
    assert len(set(restated("side_wide_u16")[1])) == 16                            # no two chunks alike: a misplaced one shows
    types = ref.filter_rows(*ref.image_bytes(tall)[:2])[1]
    assert {0, 2} <= set(types.tolist())                                           # one-byte rows: None and Up both win rows


def test_the_fibonacci_histogram_needs_the_length_limit():
    lit = np.zeros(ref.N_LITLEN, np.int64)
    lit[256] = 1
    for s in symbols_of(IMAGES["fibonacci"])[0]:
        lit[s[0] if len(s) == 1 else ref._length_symbol(s[0])[0]] += 1
    info = {}
    lengths = ref.code_lengths(lit, info)
    assert info["unlimited"] > ref.MAX_BITS and lengths.max() == ref.MAX_BITS
    assert sum(2.0 ** -int(v) for v in lengths if v) == 1.0                        # still a complete code


def test_code_lengths_of_degenerate_alphabets():
    assert ref.code_lengths([0] * 30).tolist() == [1] + [0] * 29
    assert ref.code_lengths([0, 0, 7, 0]).tolist() == [0, 0, 1, 0]
    assert ref.code_lengths([5, 0, 7, 0]).tolist() == [1, 0, 1, 0]
    assert ref.canonical_codes([2, 1, 3, 3]) == [2, 0, 6, 7]                       # RFC 1951 3.2.2's example shape


def test_adler_partials_combine_to_zlibs_adler32():
    data = np.random.default_rng(3).integers(0, 256, 3 * ref.CHUNK + 1234).astype(np.uint8).tobytes()
    parts = [ref.adler_partial(data[o:o + ref.CHUNK]) for o in range(0, len(data), ref.CHUNK)]
    want = zlib.adler32(data) & 0xFFFFFFFF
    assert ref.adler_combine([p + (min(ref.CHUNK, len(data) - k * ref.CHUNK),) for k, p in enumerate(parts)]) == want
    assert pngenc.adler_combine(parts, len(data)) == want


def test_the_packages_framing_is_the_restatements():
    img = IMAGES["c3_u16"]
    deflated, parts = ref.deflate(img)
    adler = pngenc.adler_combine([p[:2] for p in parts], sum(p[2] for p in parts))
    assert pngenc.assemble(37, 53, 3, 2, deflated, adler) == png_of("c3_u16")
    assert pngenc.n_chunks(513, 255, 1, 1) == 3 and pngenc.filtered_bytes(37, 53, 3, 2) == 37 * (1 + 53 * 6)


def test_mode_from_env(monkeypatch):
    monkeypatch.delenv("GS360_PNG_ENCODER", raising=False)
    assert pngenc.mode_from_env() is False
    monkeypatch.setenv("GS360_PNG_ENCODER", "device")
    assert pngenc.mode_from_env() is True
    monkeypatch.setenv("GS360_PNG_ENCODER", "gpu")
    with pytest.raises(ValueError):
        pngenc.mode_from_env()


def test_bound_is_host_only_and_checks_its_arguments():
    assert pngenc.bound(1, 1, 3, 1) == 2 * 4 + 176
    assert pngenc.bound(513, 255, 1, 1) == 2 * (2 * ref.CHUNK + 256) + 3 * 176
    from gs360 import capi
    for bad in ((0, 1, 3, 1), (1, 70000, 3, 1), (1, 1, 2, 1), (1, 1, 3, 4)):
        with pytest.raises(capi.Gs360Error):
            pngenc.bound(*bad)


def host_png_size(img, tmp_path):
    path = tmp_path / "host.png"
    imageio.write_image(path, img)
    return path.stat().st_size


def check_size_conditions(encode, tmp_path):
    """the issue's size conditions on the two seeded fixtures, for any encoder (the restatement here, the device in the GPU test)"""
    for dtype in (np.uint8, np.uint16):
        img = cases.photo_fixture(dtype)
        ours, host = len(encode(img)), host_png_size(img, tmp_path)
        print(f"photo fixture {np.dtype(dtype).name}: {ours} bytes, host writer {host} ({ours / host:.3f})")
        assert ours <= host
    mask = cases.mask_fixture()
    ours, host = len(encode(mask)), host_png_size(mask, tmp_path)
    print(f"mask fixture: {ours} bytes = {100.0 * ours / mask.size:.2f} % of raw, host writer {host} ({ours / host:.3f})")
    assert ours <= 0.04 * mask.size


def test_size_conditions(tmp_path):
    check_size_conditions(ref.encode, tmp_path)
