"""4:2:2, 4:4:0 and 4:1:1 files on the CPU: the NumPy restatement (tests/jpegsamp_np.py: libjpeg's h2v1 and h1v2 "fancy" upsampling and
the plain replication of h4v1) equals Pillow byte for byte on the matrix of tests/jpegsamp_cases.py; gs360.jpegdec.parse() keeps
refusing those layouts by default and accepts them, with the right geometry, under samplings=DEVICE_SAMPLINGS; the C ABI sizes their
scratch and the encoder still refuses them."""
import ctypes as ct

import numpy as np
import pytest

pytest.importorskip("PIL.Image")

from gs360 import capi, jpegdec  # noqa: E402

import jpegdec_cases as cases  # noqa: E402
import jpegsamp_cases as sc  # noqa: E402
import jpegsamp_np as samp  # noqa: E402

CHUNKS = 16
ERR_ARG, ERR_UNSUPPORTED = -1, -4        # GS360_ERR_ARG, GS360_ERR_UNSUPPORTED
CONSTANTS = {"4:2:2": capi.JPEG_422, "4:4:0": capi.JPEG_440, "4:1:1": capi.JPEG_411}
# mode -> (MCU height, MCU width, blocks per MCU)
GEOMETRY = {"4:2:2": (8, 16, 4), "4:4:0": (16, 8, 4), "4:1:1": (8, 32, 6)}


def test_the_constants_are_the_headers():
    assert (capi.JPEG_444, capi.JPEG_422, capi.JPEG_420, capi.JPEG_440, capi.JPEG_411) == (0, 1, 2, 3, 4)


@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_restatement_equals_pillow(chunk):
    matrix = sc.matrix()
    assert len(matrix) == 3 * 78 + 234
    for name, data in matrix[chunk::CHUNKS]:
        assert np.array_equal(samp.decode(data), cases.pillow(data)), name


def test_restatement_equals_the_v1_restatement_on_420_and_444():
    """the control: the general decoder is tests/jpegdec_np.py on the layouts that one takes"""
    import jpegdec_np as ref
    for sub in (0, 2):
        data = cases.encode(cases.image(37, 53, "noise"), quality=90, subsampling=sub)
        assert np.array_equal(samp.decode(data), ref.decode(data))
    data = samp.write(cases.image(37, 53, "noise"), 2, 2, 90, 3)
    assert np.array_equal(samp.decode(data), ref.decode(data)) and np.array_equal(ref.decode(data), cases.pillow(data))


def _patched(data, sampling):
    """the file with its three SOF0 sampling bytes replaced"""
    at = data.index(b"\xff\xc0") + 10
    out = bytearray(data)
    for k, s in enumerate(sampling):
        assert out[at + 3 * k] == k + 1
        out[at + 3 * k + 1] = s
    return bytes(out)


@pytest.mark.parametrize("mode", sc.MODES)
def test_parse_takes_the_layout_only_when_asked(mode):
    hs, vs = samp.SAMPLINGS[mode]
    mcu_h, mcu_w, bpm = GEOMETRY[mode]
    for h, w in ((37, 53), (64, 129), (1, 1)):
        data = samp.write(cases.image(h, w, "smooth"), hs, vs, 90, 0)
        with pytest.raises(jpegdec.Unsupported, match="sampling factors %d%d,11,11" % (hs, vs)):
            jpegdec.parse(data)
        with pytest.raises(jpegdec.Unsupported):
            jpegdec.parse(data, samplings=jpegdec.V1_SAMPLINGS)
        d = jpegdec.parse(data, samplings=jpegdec.DEVICE_SAMPLINGS)
        assert (d.H, d.W, d.C, d.subsampling) == (h, w, 3, CONSTANTS[mode])
        assert d.luma_sampling == (hs, vs) and d.mcu_px == (mcu_h, mcu_w) == (d.mcu_h, d.mcu_w) and d.blocks_per_mcu == bpm
        assert d.mcu_grid == (-(-h // mcu_h), -(-w // mcu_w)) and d.n_mcu == -(-h // mcu_h) * -(-w // mcu_w)
        assert d.segments.shape == (1, 2) and d.restart == 0


def test_parse_keeps_the_old_layouts_geometry():
    for sub, px, bpm in ((0, 8, 3), (2, 16, 6)):
        data = cases.encode(cases.image(37, 53, "noise"), quality=90, subsampling=sub)
        for kw in ({}, {"samplings": jpegdec.DEVICE_SAMPLINGS}):
            d = jpegdec.parse(data, **kw)
            assert d.subsampling == sub and d.mcu_px == (px, px) and d.blocks_per_mcu == bpm
            assert d.mcu_grid == (-(-37 // px), -(-53 // px)) and d.n_mcu == d.mcu_grid[0] * d.mcu_grid[1]
    d = jpegdec.parse(cases.encode(cases.image(37, 53, "noise", gray=True), quality=90), samplings=jpegdec.DEVICE_SAMPLINGS)
    assert d.mcu_px == (8, 8) and d.blocks_per_mcu == 1 and d.n_mcu == 5 * 7


def test_parse_still_refuses_other_factor_sets():
    good = cases.encode(cases.image(48, 80, "noise"), quality=90, subsampling=1)
    assert jpegdec.parse(good, samplings=jpegdec.DEVICE_SAMPLINGS).subsampling == capi.JPEG_422
    for sampling in ((0x22, 0x21, 0x21), (0x42, 0x11, 0x11), (0x21, 0x11, 0x21), (0x21, 0x12, 0x11), (0x14, 0x11, 0x11)):
        for kw in ({}, {"samplings": jpegdec.DEVICE_SAMPLINGS}):
            with pytest.raises(jpegdec.Unsupported, match="sampling factors"):
                jpegdec.parse(_patched(good, sampling), **kw)
    from PIL import Image
    import io
    f = io.BytesIO()
    Image.fromarray(cases.image(48, 80, "noise")).convert("CMYK").save(f, "JPEG", quality=90)
    with pytest.raises(jpegdec.Unsupported, match="4 components"):
        jpegdec.parse(f.getvalue(), samplings=jpegdec.DEVICE_SAMPLINGS)


def test_segment_table_of_a_411_file_with_a_partial_last_interval():
    data = samp.write(cases.image(20, 100, "noise"), 4, 1, 100, 5)       # 3 x 4 MCUs of 32 x 8 in intervals of 5: 5, 5, 2
    d = jpegdec.parse(data, samplings=jpegdec.DEVICE_SAMPLINGS)
    assert d.mcu_grid == (3, 4) and d.n_mcu == 12 and d.restart == 5 and d.segments.shape == (3, 2)
    table, n_sub = jpegdec.segment_table(d)
    per = -(-d.segments[:, 1].astype(np.int64) // jpegdec.subseq_bytes())
    assert per.max() > 1                                                 # (noise at quality 100: an interval takes several subsequences)
    assert list(table[:, 3]) == [0, 5, 10]
    assert list(table[:, 2]) == list(np.cumsum(per) - per) and n_sub == per.sum()
    assert list(table[:, 0]) == list(d.segments[:, 0]) and list(table[:, 1]) == list(d.segments[:, 1])
    assert np.array_equal(samp.decode(data), cases.pillow(data))


@pytest.fixture(scope="module")
def lib():
    if not capi.LIB_PATH.exists():
        pytest.skip("libgs360hip.so not built (run __graft_entry__.build())")
    return capi.load_library()


def _scratch(lib, h, w, c, sub, n_sub):
    n = ct.c_size_t(0)
    rc = lib.gs360_jpeg_decode_scratch(h, w, c, sub, n_sub, ct.byref(n))
    return rc, int(n.value)


def test_decode_scratch_takes_the_new_constants(lib):
    for sub in (capi.JPEG_422, capi.JPEG_440, capi.JPEG_411):
        rc, small = _scratch(lib, 100, 150, 3, sub, 10)
        rc2, large = _scratch(lib, 100, 150, 3, sub, 1000)
        assert rc == rc2 == 0 and 0 < small < large
        assert _scratch(lib, 100, 150, 1, sub, 10) == _scratch(lib, 100, 150, 1, capi.JPEG_444, 10)       # gray ignores it
    # equal block counts (6 blocks, 4 of them luma) give equal layouts: 4:1:1 32 x 8 and 4:2:0 16 x 16; and 4 blocks: 4:2:2 16 x 8, 4:4:0 8 x 16
    assert _scratch(lib, 8, 32, 3, capi.JPEG_411, 7) == _scratch(lib, 16, 16, 3, capi.JPEG_420, 7)
    assert _scratch(lib, 8, 16, 3, capi.JPEG_422, 7) == _scratch(lib, 16, 8, 3, capi.JPEG_440, 7)
    # the coefficients dominate: 128 bytes per block, 4 blocks per 128 pixels (4:2:2, 4:4:0) or 6 per 256 (4:1:1)
    for sub, blocks in ((capi.JPEG_422, 4 * 16 * 64), (capi.JPEG_440, 4 * 32 * 32), (capi.JPEG_411, 6 * 8 * 64)):
        rc, n = _scratch(lib, 512, 256, 3, sub, 1)
        assert rc == 0 and blocks * 132 <= n <= blocks * 132 + 8 * 256
    assert _scratch(lib, 100, 150, 3, 5, 10)[0] == ERR_UNSUPPORTED and _scratch(lib, 100, 150, 3, -1, 10)[0] == ERR_UNSUPPORTED


def test_the_encoder_still_refuses_the_new_constants(lib):
    n = ct.c_size_t(0)
    assert lib.gs360_jpeg_scan_bound_sub(64, 64, 3, 8, capi.JPEG_420, ct.byref(n)) == 0
    for sub in (capi.JPEG_422, capi.JPEG_440, capi.JPEG_411):
        assert lib.gs360_jpeg_scan_bound_sub(64, 64, 3, 8, sub, ct.byref(n)) == ERR_ARG
