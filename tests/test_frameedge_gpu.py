"""gs360_frame_edge_u8 on the MI355X against the FS-EDGE v1 restatement (tests/frameedge_np.py): all three int64 fields exactly, and
the default backend's 9-tuple through gs360.framescore's drop-in seams."""
import ctypes

import numpy as np
import pytest

import frame_layouts as layouts
import frameedge_np as enp
from gs360 import framescore

pytestmark = pytest.mark.gpu


def _frame(rng, H, W, C, kind):
    yy, xx = np.mgrid[:H, :W]
    if kind == "noise":
        g = rng.integers(0, 256, size=(H, W))
    elif kind == "constant":
        g = np.full((H, W), 77)
    elif kind == "vstep":
        g = np.where(xx >= W // 2, 255, 0)
    elif kind == "hstep":
        g = np.where(yy >= H // 2, 60, 0)
    else:                                               # ramp: reaches the last column and the last row
        g = (3 * xx + 5 * yy) % 256
    g = g.astype(np.uint8)
    if C == 1:
        return g
    return np.ascontiguousarray(np.repeat(g[:, :, None], C, axis=2) ^ (np.arange(C, dtype=np.uint8) * 17))


def _run(ctx, frames, band, red_index=0, pad=0, window=None):
    """The records of one call; pad > 0 uploads every frame with `pad` bytes of filler after each row and passes the stride,
    window = (parent_h, parent_w, row, col) places every frame inside a parent image (frame_layouts.upload)."""
    H, W = frames[0].shape[:2]
    Cn = layouts.channels(frames[0])
    objs, stride, bufs = layouts.upload(ctx, frames, pad, window)
    out = ctx.alloc(len(frames) * 24)
    try:
        ctx.memset(out, 0x5A)                          # the call clears the records itself
        ctx.frame_edge_dev(objs, H, W, Cn, band, out, red_index=red_index, stride=stride)
        ctx.sync(0)
        recs = ctx.download(out, (len(frames), 3), np.int64)
    finally:
        for b in bufs + [out]:
            ctx.free(b)
    return [dict(zip(enp.FIELDS, map(int, r))) for r in recs]


CASES = [  # H, W, C, red_index, crop, pad, kind
    (37, 45, 3, 0, 0.8, 0, "noise"), (37, 45, 3, 2, 0.6, 0, "ramp"), (64, 63, 1, 0, 1.0, 0, "noise"), (50, 17, 4, 2, 0.8, 0, "noise"),
    (33, 1, 3, 0, 0.8, 0, "noise"), (1, 70, 1, 0, 0.8, 0, "noise"), (2, 2, 4, 0, 1.0, 0, "noise"), (1, 1, 1, 0, 1.0, 0, "noise"),
    (40, 255, 3, 0, 0.8, 0, "noise"), (40, 256, 3, 2, 0.8, 0, "ramp"), (40, 257, 3, 0, 0.8, 0, "noise"), (40, 513, 1, 0, 0.8, 0, "ramp"),
    (40, 513, 3, 0, 0.8, 7, "noise"), (40, 257, 4, 0, 0.8, 4, "noise"), (40, 255, 1, 0, 0.8, 1, "ramp"), (21, 300, 3, 2, 1.0, 13, "vstep"),
    (15, 90, 3, 0, 1.0, 0, "noise"), (16, 90, 3, 0, 1.0, 0, "ramp"), (17, 90, 3, 0, 1.0, 0, "noise"), (33, 90, 1, 0, 1.0, 0, "ramp"),
    (48, 300, 3, 0, 1.0, 0, "constant"), (48, 300, 3, 0, 1.0, 0, "vstep"), (48, 300, 1, 0, 1.0, 0, "hstep"), (48, 300, 4, 0, 0.8, 0, "vstep"),
    (129, 513, 3, 2, 0.8, 0, "ramp"), (600, 257, 1, 0, 0.6, 0, "noise"), (96, 600, 4, 0, 0.8, 0, "ramp")]


@pytest.mark.parametrize("H,W,C,red,crop,pad,kind", CASES)
def test_fields_equal_the_restatement(ctx, H, W, C, red, crop, pad, kind):
    rng = np.random.default_rng(H * 1000 + W + C)
    img = _frame(rng, H, W, C, kind)
    band = framescore.edge_band_rows(H, crop)
    got = _run(ctx, [img], band, red, pad)
    assert got[0] == enp.frame_edge(img, *band, red)


@pytest.mark.parametrize("kind", ["noise", "ramp"])
def test_bands_inside_strips_and_one_row_bands(ctx, kind):
    rng = np.random.default_rng(5)
    img = _frame(rng, 70, 300, 3, kind)
    for band in [(0, 1), (17, 18), (69, 70), (15, 16), (16, 17), (3, 9), (5, 37), (16, 32), (15, 33), (1, 69), (31, 70), (20, 22)]:
        assert _run(ctx, [img], band)[0] == enp.frame_edge(img, *band), band


@pytest.mark.parametrize("n", [1, 16, 17])
def test_batches(ctx, n):
    rng = np.random.default_rng(100 + n)
    frames = [_frame(rng, 61, 270, 3, ("noise", "ramp", "vstep")[k % 3]) for k in range(n)]
    band = framescore.edge_band_rows(61, 0.8)
    got = _run(ctx, frames, band)
    for k, f in enumerate(frames):
        assert got[k] == enp.frame_edge(f, *band), k


def test_one_8k_frame_sums_past_32_bits(ctx):
    rng = np.random.default_rng(8)
    H, W = 3840, 7680
    img = rng.integers(150, 256, size=(H, W, 3), dtype=np.uint8)
    band = framescore.edge_band_rows(H, 0.8)
    got = _run(ctx, [img], band)[0]
    assert got["sum_gray"] > 2 ** 32
    assert got == enp.frame_edge(img, *band)


def test_argument_errors_return_their_codes_without_a_launch(ctx):
    H, W = 20, 30
    buf = ctx.to_device(np.zeros((H, W, 3), np.uint8))
    out = ctx.alloc(24)
    fn = ctx.L.gs360_frame_edge_u8
    one = (ctypes.c_void_p * 1)(buf.ptr)

    def call(frames=one, n=1, h=H, w=W, c=3, stride=0, red=0, y0=2, y1=18, o=None, slot=0):
        return fn(ctx.handle, frames, n, h, w, c, stride, red, y0, y1, out.ptr if o is None else o, slot)
    try:
        ctx.memset(out, 0x5A)
        ctx.sync(0)
        ARG, UNSUPPORTED = -1, -4
        assert call(n=-1) == ARG
        assert call(frames=None) == ARG
        assert call(o=ctypes.c_void_p(None)) == ARG
        assert call(c=2) != 0
        assert call(red=1) == ARG
        assert call(h=0) == ARG
        assert call(h=65536, y1=18) == UNSUPPORTED
        assert call(w=65536) == UNSUPPORTED
        assert call(stride=W * 3 - 1) == ARG
        assert call(y0=-1) == ARG
        assert call(y1=H + 1) == ARG
        assert call(y0=5, y1=5) == ARG
        assert call(frames=(ctypes.c_void_p * 1)(None)) == ARG
        assert call(frames=(ctypes.c_void_p * 1)(buf.ptr + 1)) == ARG
        assert call(slot=99) == ARG
        ctx.sync(0)
        assert np.all(ctx.download(out, (24,), np.uint8) == 0x5A)          # nothing ran: not even the clearing of the records
        assert call(n=0) == 0
        assert call() == 0
        ctx.sync(0)
        assert ctx.download(out, (3,), np.int64).tolist() == [W * 16, 0, 0]
    finally:
        ctx.free(buf)
        ctx.free(out)


def test_default_backend_through_the_seams(ctx, tmp_path):
    """score_one_record with score_backend="ffmpeg" (the reference CLI's default) is the edge pass, whatever the metric."""
    from gs360 import imageio
    rng = np.random.default_rng(7)
    x = _frame(rng, 300, 700, 3, "ramp")
    y = (_frame(rng, 300, 700, 3, "noise") // 4).astype(np.uint8)            # dark: the penalty branch
    imageio.write_image(tmp_path / "x.png", x)
    imageio.write_image(tmp_path / "y.png", y)
    for img, name in ((x, "x.png"), (y, "y.png")):
        rec = {"input_mode": "single", "file_paths": [str(tmp_path / name)]}
        assert framescore.score_one_record(rec, "hybrid", 0.8, 0, False, True, "ffmpeg") == enp.score(img, 0.8)
        assert framescore.score_one_file_ffmpeg(str(tmp_path / name), "lapvar", 1.0, 0, True, False) == enp.score(img, 1.0)
    assert enp.score(y, 0.8)[4] < 1.0
    paths = [str(tmp_path / "x.png"), str(tmp_path / "nope.png"), str(tmp_path / "y.png")]
    got = framescore.score_files(paths, "hybrid", 0.8, 0, False, True, backend="ffmpeg")
    assert got == [enp.score(x, 0.8), framescore.FAILED, enp.score(y, 0.8)]
    # a pair record keeps the OpenCV path under the circle mask (FS:480-483)
    pair = {"input_mode": "pair", "file_paths": paths[::2]}
    assert framescore.score_one_record(pair, "lapvar", 0.8, 0, False, True, "ffmpeg") == \
        framescore.score_one_record(pair, "lapvar", 0.8, 0, False, True, "opencv")
    assert framescore.score_one_file_ffmpeg(paths[0], "lapvar", 0.8, 0, False, True, "fisheye_circle") == \
        framescore.score_one_file(paths[0], "lapvar", 0.8, 0, False, True, "fisheye_circle")


def test_device_frames_take_the_edge_pass_without_a_round_trip(ctx):
    rng = np.random.default_rng(11)
    img = _frame(rng, 200, 640, 3, "ramp")
    buf = ctx.to_device(img)
    try:
        got = framescore.edge_arrays(ctx, [framescore.DeviceFrame(buf, 200, 640, 3)], 0.8)
    finally:
        ctx.free(buf)
    assert got == [enp.score(img, 0.8)]


@pytest.mark.parametrize("pad", [1, 2, 3])
def test_maximal_staging_on_odd_strides(ctx, pad):
    H, W, C = layouts.MAXIMAL
    layouts.check_maximal_staging(pad)
    img = _frame(np.random.default_rng(514 + pad), H, W, C, "noise")
    assert _run(ctx, [img], layouts.MAXIMAL_BAND, pad=pad)[0] == enp.frame_edge(img, *layouts.MAXIMAL_BAND)


@pytest.mark.parametrize("C", [1, 3, 4])
def test_windows_of_a_parent_image(ctx, C):
    """A 37 x 515 window at row 5 of a 64 x 640 parent: the band and the mirrored halo are the window's own."""
    H, W, PH, PW, row = 37, 515, 64, 640, 5
    col = layouts.window_column(9, PW * C, row, C)
    for kind in ("noise", "ramp"):
        img = _frame(np.random.default_rng(515 + C), H, W, C, kind)
        for crop in (0.8, 1.0):
            band = framescore.edge_band_rows(H, crop)
            assert _run(ctx, [img], band, window=(PH, PW, row, col))[0] == enp.frame_edge(img, *band), (kind, crop)


def test_device_frames_of_three_strides_in_one_call(ctx):
    """DeviceFrames of one shape stored packed (stride 0 and W*C) and with 8 filler bytes a row: each is read with its own stride."""
    rng = np.random.default_rng(61)
    frames = [_frame(rng, 61, 90, 3, ("noise", "ramp", "vstep")[k % 3]) for k in range(6)]
    dev, bufs = layouts.mixed_strides(ctx, frames)
    try:
        got = framescore.edge_arrays(ctx, dev, 0.8)
    finally:
        for b in bufs:
            ctx.free(b)
    assert got == framescore.edge_arrays(ctx, frames, 0.8) == [enp.score(f, 0.8) for f in frames]
