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
