"""gs360_frame_stats_u8 on the MI355X against the FS-SPEC v1 restatement (tests/framescore_np.py): every int64 field exactly, the
INTER_AREA fft input within 1e-5 relative, and the 9-tuples of gs360.framescore's drop-in seams."""
import numpy as np
import pytest

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


def _run(ctx, frames, band, flags, red_index=0, small=None):
    H, W = frames[0].shape[:2]
    Cn = 1 if frames[0].ndim == 2 else frames[0].shape[2]
    bufs = [ctx.to_device(f) for f in frames]
    stats = ctx.alloc(len(frames) * 104)
    smalls = [ctx.alloc(2 * small[0] * small[1] * 4) for _ in frames] if small else None
    try:
        ctx.frame_stats_dev(bufs, H, W, Cn, band, stats, flags=flags, smalls=smalls, small_w=small[0] if small else 0,
                            small_h=small[1] if small else 0, red_index=red_index)
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
