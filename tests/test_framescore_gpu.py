"""gs360_frame_stats_u8 on the MI355X against the FS-SPEC v1 restatement (tests/framescore_np.py): every int64 field exactly, the
INTER_AREA fft input within 1e-5 relative, and the 9-tuples of gs360.framescore's drop-in seams."""
import ctypes

import numpy as np
import pytest

import frame_layouts as layouts
import framescore_np as fnp
from gs360 import capi, framescore

pytestmark = pytest.mark.gpu


def _frame(rng, H, W, C, kind):
    shape = (H, W) if C == 1 else (H, W, C)
    if kind == "random":
        return rng.integers(0, 256, size=shape, dtype=np.uint8)
    if kind == "black":
        return np.zeros(shape, np.uint8)
    if kind == "white":
        return np.full(shape, 255, np.uint8)
    yy, xx = np.mgrid[:H, :W]               # structured: ramps, a disc of highlights and a little noise
    g = (xx * 7 + yy * 3) % 256
    g = np.where((xx - W / 3) ** 2 + (yy - H / 2) ** 2 < (min(H, W) / 4) ** 2, 250, g)
    g = np.clip(g + rng.integers(-3, 4, size=g.shape), 0, 255).astype(np.uint8)
    return g if C == 1 else np.repeat(g[:, :, None], C, axis=2) ^ np.arange(C, dtype=np.uint8) * 17


def _run(ctx, frames, band, flags, red_index=0, small=None, pad=0, window=None):
    """The records (and fft-input planes) of one call on frames laid out as frame_layouts.upload makes them; the records are
    filled with 0x5A first: the call clears them itself."""
    H, W = frames[0].shape[:2]
    Cn = layouts.channels(frames[0])
    objs, stride, bufs = layouts.upload(ctx, frames, pad, window)
    stats = ctx.alloc(len(frames) * 104)
    smalls = [ctx.alloc(2 * small[0] * small[1] * 4) for _ in frames] if small else None
    try:
        ctx.memset(stats, 0x5A)
        ctx.frame_stats_dev(objs, H, W, Cn, band, stats, flags=flags, smalls=smalls, small_w=small[0] if small else 0,
                            small_h=small[1] if small else 0, red_index=red_index, stride=stride)
        ctx.sync(0)
        recs = ctx.download(stats, (len(frames), 13), np.int64)
        planes = [ctx.download(b, (2, small[1], small[0]), np.float32) for b in smalls] if small else None
    finally:
        for b in bufs + [stats] + (smalls or []):
            ctx.free(b)
    return [dict(zip(fnp.FIELDS, map(int, r))) for r in recs], planes


def _check_small(img, band, plane, red_index=0):
    area, near = fnp.fft_input(img, band[0], band[1], red_index)
    np.testing.assert_allclose(plane[0], area, rtol=1e-5, atol=1e-4)
    assert np.array_equal(plane[1], near)


CASES = [  # H, W, C, red_index, crop, kind
    (37, 45, 3, 0, 0.8, "random"), (37, 45, 3, 2, 0.6, "structured"), (64, 63, 1, 0, 1.0, "random"), (50, 17, 4, 2, 0.8, "random"),
    (33, 1, 3, 0, 0.8, "random"), (1, 70, 1, 0, 0.8, "random"), (2, 2, 4, 0, 1.0, "random"), (40, 300, 3, 0, 0.8, "white"),
    (40, 300, 3, 0, 0.8, "black"), (129, 513, 3, 2, 0.8, "structured"), (600, 257, 1, 0, 0.6, "structured"),
    (96, 600, 4, 0, 0.8, "structured")]


@pytest.mark.parametrize("H,W,C,red,crop,kind", CASES)
@pytest.mark.parametrize("flags", [0, capi.FS_CIRCLE, capi.FS_HIGHLIGHTS, capi.FS_CIRCLE | capi.FS_HIGHLIGHTS])
def test_fields_equal_the_restatement(ctx, H, W, C, red, crop, kind, flags):
    rng = np.random.default_rng(H * 1000 + W + C)
    img = _frame(rng, H, W, C, kind)
    band = framescore.band_rows(H, crop)
    small = framescore.fft_input_size(W, band[1] - band[0])
    got, planes = _run(ctx, [img], band, flags, red, small)
    assert got[0] == fnp.frame_stats(img, *band, bool(flags & capi.FS_CIRCLE), bool(flags & capi.FS_HIGHLIGHTS), red)
    _check_small(img, band, planes[0], red)


def test_one_row_bands(ctx):
    rng = np.random.default_rng(5)
    img = _frame(rng, 48, 70, 3, "random")
    for band in [(0, 1), (17, 18), (47, 48), (15, 16), (16, 17)]:
        got, _ = _run(ctx, [img], band, capi.FS_CIRCLE)
        assert got[0] == fnp.frame_stats(img, *band, True, False), band


@pytest.mark.parametrize("n", [1, 7, 16, 17])
def test_batches(ctx, n):
    rng = np.random.default_rng(100 + n)
    frames = [_frame(rng, 61, 90, 3, "random" if k % 2 else "structured") for k in range(n)]
    band = framescore.band_rows(61, 0.8)
    got, planes = _run(ctx, frames, band, capi.FS_HIGHLIGHTS, small=(90, band[1] - band[0]))
    for k, f in enumerate(frames):
        assert got[k] == fnp.frame_stats(f, *band, False, True), k
        _check_small(f, band, planes[k])


def test_full_size_batch_of_16_8k_frames(ctx):
    rng = np.random.default_rng(8)
    H, W = 3840, 7680
    base = _frame(rng, H, W, 3, "structured")
    frames = [np.roll(base, 97 * k, axis=1) ^ rng.integers(0, 8, size=(1, W, 3), dtype=np.uint8) for k in range(16)]
    band = framescore.band_rows(H, 0.8)
    small = framescore.fft_input_size(W, band[1] - band[0])
    got, planes = _run(ctx, frames, band, capi.FS_HIGHLIGHTS, small=small)
    assert len({tuple(g.values()) for g in got}) == 16          # distinct frames, distinct records
    for k in (0, 9, 15):
        assert got[k] == fnp.frame_stats(frames[k], *band, False, True), k
        _check_small(frames[k], band, planes[k])


def test_fisheye_pair_3840(ctx):
    rng = np.random.default_rng(3840)
    pair = [_frame(rng, 3840, 3840, 3, "structured"), _frame(rng, 3840, 3840, 3, "random")]
    got = framescore.score_arrays(ctx, pair, "hybrid", 0.8, True, True, "fisheye_circle")
    for g, img in zip(got, pair):
        _assert_tuple(g, fnp.score(img, "hybrid", 0.8, True, True, "fisheye_circle"))


def _assert_tuple(got, want):
    assert len(got) == 9
    for k, (a, b) in enumerate(zip(got, want)):
        if k in (0, 7) and a is not None and b is not None:        # sharp and the fft feature carry the float32 INTER_AREA image
            assert a == pytest.approx(b, rel=1e-5), k
        else:
            assert a == b, k


@pytest.mark.parametrize("metric", ["lapvar", "tenengrad", "fft", "hybrid"])
def test_score_one_file_and_record(ctx, tmp_path, metric):
    from gs360 import imageio
    rng = np.random.default_rng(7)
    x = _frame(rng, 300, 700, 3, "structured")
    y = _frame(rng, 300, 700, 3, "random")
    imageio.write_image(tmp_path / "x.png", x)
    imageio.write_image(tmp_path / "y.png", y)
    got = framescore.score_one_file(str(tmp_path / "x.png"), metric, 0.8, 0, True, True)
    _assert_tuple(got, fnp.score(x, metric, 0.8, True, True))
    rec = {"input_mode": "pair", "file_paths": [str(tmp_path / "x.png"), str(tmp_path / "y.png")]}
    got = framescore.score_one_record(rec, metric, 0.8, 0, False, True, "opencv")
    want = [fnp.score(a, metric, 0.8, False, True, "fisheye_circle") for a in (x, y)]
    avg = [None if want[0][k] is None else (want[0][k] + want[1][k]) / 2.0 for k in range(9)]
    _assert_tuple(got, tuple(avg))
    assert framescore.score_files([str(tmp_path / "x.png"), str(tmp_path / "nope.png")], metric, 0.8, 0, True, False)[1] == \
        framescore.FAILED


def test_device_frames_score_without_a_round_trip(ctx):
    rng = np.random.default_rng(11)
    img = _frame(rng, 200, 640, 3, "structured")
    buf = ctx.to_device(img)
    try:
        got = framescore.score_arrays(ctx, [framescore.DeviceFrame(buf, 200, 640, 3)], "hybrid", 0.8, True, False)
    finally:
        ctx.free(buf)
    _assert_tuple(got[0], fnp.score(img, "hybrid", 0.8, True, False))


# ---- row strides, windows and strip seams ---------------------------------------------------------------------------------------
ALL_FLAGS = [0, capi.FS_CIRCLE, capi.FS_HIGHLIGHTS, capi.FS_CIRCLE | capi.FS_HIGHLIGHTS]


@pytest.mark.parametrize("pad", [1, 2, 3])
def test_maximal_staging_on_odd_strides(ctx, pad):
    H, W, C = layouts.MAXIMAL
    band = layouts.MAXIMAL_BAND
    layouts.check_maximal_staging(pad)
    img = _frame(np.random.default_rng(514 + pad), H, W, C, "random")
    got, _ = _run(ctx, [img], band, capi.FS_CIRCLE | capi.FS_HIGHLIGHTS, pad=pad)
    assert got[0] == fnp.frame_stats(img, *band, True, True)


@pytest.mark.parametrize("H,W,C,pad", [(33, 257, 3, 5), (17, 255, 1, 3), (40, 300, 3, 1), (37, 45, 4, 2), (2, 2, 4, 6), (33, 1, 3, 1)])
@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_padded_rows(ctx, H, W, C, pad, flags):
    img = _frame(np.random.default_rng(H * 1000 + W + C + pad), H, W, C, "random" if pad % 2 else "structured")
    band = framescore.band_rows(H, 0.8)
    small = framescore.fft_input_size(W, band[1] - band[0])
    for red in (0, 2):
        got, planes = _run(ctx, [img], band, flags, red, small, pad=pad)
        assert got[0] == fnp.frame_stats(img, *band, bool(flags & capi.FS_CIRCLE), bool(flags & capi.FS_HIGHLIGHTS), red), red
        _check_small(img, band, planes[0], red)


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_windows_of_a_parent_image(ctx, C, flags):
    """A 37 x 515 window at row 5 of a 64 x 640 parent: the circle, the band and the reflected halo are the window's own."""
    H, W, PH, PW, row = 37, 515, 64, 640, 5
    col = layouts.window_column(9, PW * C, row, C)
    img = _frame(np.random.default_rng(515 + C), H, W, C, "structured")
    band = framescore.band_rows(H, 0.8)
    small = framescore.fft_input_size(W, band[1] - band[0])
    got, planes = _run(ctx, [img], band, flags, 0, small, window=(PH, PW, row, col))
    assert got[0] == fnp.frame_stats(img, *band, bool(flags & capi.FS_CIRCLE), bool(flags & capi.FS_HIGHLIGHTS))
    _check_small(img, band, planes[0])


@pytest.mark.parametrize("kind", ["random", "structured"])
def test_bands_against_strip_seams(ctx, kind):
    img = _frame(np.random.default_rng(5), 70, 300, 3, kind)
    for band in [(0, 1), (17, 18), (69, 70), (15, 16), (16, 17), (3, 9), (5, 37), (16, 32), (15, 33), (1, 69), (31, 70), (20, 22)]:
        for flags in (0, capi.FS_CIRCLE | capi.FS_HIGHLIGHTS):
            got, _ = _run(ctx, [img], band, flags)
            assert got[0] == fnp.frame_stats(img, *band, bool(flags), bool(flags)), (band, flags)


def test_argument_errors_return_their_codes_without_a_launch(ctx):
    H, W = 20, 30
    buf = ctx.to_device(np.zeros((H, W, 3), np.uint8))
    out = ctx.alloc(104)
    plane = ctx.alloc(2 * W * 16 * 4)
    fn = ctx.L.gs360_frame_stats_u8
    one = (ctypes.c_void_p * 1)(buf.ptr)
    sm = (ctypes.c_void_p * 1)(plane.ptr)

    def call(frames=one, n=1, h=H, w=W, c=3, stride=0, red=0, y0=2, y1=18, flags=0, o=None, small=None, sw=0, sh=0, slot=0):
        return fn(ctx.handle, frames, n, h, w, c, stride, red, y0, y1, flags, out.ptr if o is None else o, small, sw, sh, slot)
    try:
        ctx.memset(out, 0x5A)
        ctx.sync(0)
        ARG, UNSUPPORTED = -1, -4
        assert call(n=-1) == ARG
        assert call(frames=None) == ARG
        assert call(o=ctypes.c_void_p(None)) == ARG
        assert call(c=2) == ARG
        assert call(red=1) == ARG
        assert call(h=0) == ARG
        assert call(h=65536, y1=18) == UNSUPPORTED
        assert call(w=65536) == UNSUPPORTED
        assert call(stride=W * 3 - 1) == ARG
        assert call(y0=-1) == ARG
        assert call(y1=H + 1) == ARG
        assert call(y0=5, y1=5) == ARG
        assert call(flags=4) == ARG
        assert call(frames=(ctypes.c_void_p * 1)(None)) == ARG
        assert call(frames=(ctypes.c_void_p * 1)(buf.ptr + 1)) == ARG
        assert call(small=(ctypes.c_void_p * 1)(None), sw=W, sh=16) == ARG
        assert call(small=sm, sw=0, sh=16) == ARG
        assert call(small=sm, sw=W + 1, sh=16) == ARG
        assert call(small=sm, sw=W, sh=17) == ARG
        assert call(slot=99) == ARG
        ctx.sync(0)
        assert np.all(ctx.download(out, (104,), np.uint8) == 0x5A)         # nothing ran: not even the clearing of the records
        assert call(n=0) == 0
        assert call(small=sm, sw=W, sh=16) == 0
        ctx.sync(0)
        rec = dict(zip(fnp.FIELDS, map(int, ctx.download(out, (13,), np.int64))))
        assert rec == fnp.frame_stats(np.zeros((H, W, 3), np.uint8), 2, 18)
    finally:
        for b in (buf, out, plane):
            ctx.free(b)


def test_device_frames_of_three_strides_in_one_call(ctx):
    """DeviceFrames of one shape stored packed (stride 0 and W*C) and with 8 filler bytes a row: each is read with its own stride."""
    rng = np.random.default_rng(61)
    frames = [_frame(rng, 61, 90, 3, "random" if k % 2 else "structured") for k in range(6)]
    dev, bufs = layouts.mixed_strides(ctx, frames)
    try:
        for fft in framescore.FFT_MODES:
            for mask_mode in ("none", "fisheye_circle"):
                got = framescore.score_arrays(ctx, dev, "hybrid", 0.8, True, True, mask_mode, fft=fft)
                want = framescore.score_arrays(ctx, frames, "hybrid", 0.8, True, True, mask_mode, fft=fft)
                assert len(got) == len(frames)
                for g, w in zip(got, want):
                    _assert_tuple(g, w)
    finally:
        for b in bufs:
            ctx.free(b)
