"""FS-DEPTH16 v1 without a GPU: the GS360_FS_DEPTH16 switch, finish(unit=257), the exact model (tests/framescore16_np.py) against
the 8-bit restatement on frames that are 8-bit frames times 257, and against the reference's float32 chain."""
import numpy as np
import pytest

import framescore16_np as fnp16
import framescore_np as fnp
from gs360 import capi, frameflow, framescore

# The exact model against reference_f32 on the frames of _frames(): the largest relative difference of a 9-tuple field, measured
# when the test was written (on the smooth ramp, whose small Laplacian variance amplifies the reference's float32 rounding).  The
# assertion allows four times it: the difference is the reference's rounding, not the model's, and the margin covers other seeds.
MEASURED_F32_DIFFERENCE = 4.74e-6


def test_env_switch(monkeypatch):
    monkeypatch.delenv("GS360_FS_DEPTH16", raising=False)
    assert framescore.depth16_mode_from_env() is False
    monkeypatch.setenv("GS360_FS_DEPTH16", "off")
    assert framescore.depth16_mode_from_env() is False
    monkeypatch.setenv("GS360_FS_DEPTH16", "device")
    assert framescore.depth16_mode_from_env() is True
    monkeypatch.setenv("GS360_FS_DEPTH16", "host")
    with pytest.raises(ValueError, match="GS360_FS_DEPTH16"):
        framescore.depth16_mode_from_env()


def test_uint16_frames_are_taken_only_with_the_switch(monkeypatch):
    a = np.zeros((4, 6, 3), np.uint16)
    monkeypatch.delenv("GS360_FS_DEPTH16", raising=False)
    with pytest.raises(capi.Gs360Error, match="8-bit"):
        framescore.frame_shape(a)
    monkeypatch.setenv("GS360_FS_DEPTH16", "device")
    assert framescore.frame_shape(a) == (4, 6, 3) and framescore.frame_depth(a) == 16
    assert framescore.row_stride(a) == 36 and framescore.row_stride(a.astype(np.uint8)) == 18
    with pytest.raises(capi.Gs360Error, match="8-bit"):                      # float images stay refused
        framescore.frame_shape(np.zeros((4, 6), np.float32))
    monkeypatch.setenv("GS360_FS_DEPTH16", "yes")
    with pytest.raises(ValueError, match="GS360_FS_DEPTH16"):
        framescore.frame_shape(a)
    with pytest.raises(ValueError, match="GS360_FS_DEPTH16"):
        frameflow.flow_arrays(None, [a, a], [(0, 1)], 1.0)


def test_batches_never_mix_sample_types(monkeypatch):
    monkeypatch.setenv("GS360_FS_DEPTH16", "device")
    frames = [np.zeros((4, 6), np.uint8), np.zeros((4, 6), np.uint16), np.zeros((4, 6), np.uint16), np.zeros((4, 6), np.uint8)]
    shapes = [framescore.frame_shape(f) for f in frames]
    assert list(framescore._batches(frames, shapes)) == [(0, 1), (1, 3), (3, 4)]
    dev = framescore.DeviceFrame(None, 4, 6, 3)
    assert dev.depth == 8 and framescore.row_stride(dev) == 18
    assert framescore.row_stride(dev._replace(depth=16)) == 36 and framescore.row_stride(dev._replace(depth=16, stride=37)) == 37


def test_the_pixel_bound_is_derived_from_the_taps():
    lap_max = 8 * 65535                       # [[2,0,2],[0,-8,0],[2,0,2]] on columns of 0 and 65535 in turn
    sobel_max = 4 * 65535
    assert 2 * sobel_max ** 2 < lap_max ** 2
    assert capi.FS16_MAX_PIXELS == (2 ** 63 - 1) // lap_max ** 2
    assert capi.FS16_MAX_PIXELS * lap_max ** 2 < 2 ** 63 <= (capi.FS16_MAX_PIXELS + 1) * lap_max ** 2
    assert 7680 * 3840 <= capi.FS16_MAX_PIXELS


def test_finish_divides_by_the_unit():
    """Hand-made sums: 6 band pixels whose 16-bit sums are the 8-bit sums times 257 (and 257^2 for the squares)."""
    st8 = {"n_circle": 6, "n_highlight": 1, "n_highlight_in_circle": 1, "n": 6, "sum_gray": 700, "sum_lap": -36, "sum_lap2": 5000,
           "sum_mag2": 9100, "n_valid": 5, "sum_gray_valid": 455, "sum_lap_valid": 12, "sum_lap2_valid": 2100, "sum_mag2_valid": 4000}
    st16 = dict(st8)
    for sfx in ("", "_valid"):
        for name, k in (("sum_gray", 257), ("sum_lap", 257), ("sum_lap2", 257 * 257), ("sum_mag2", 257 * 257)):
            st16[name + sfx] = st8[name + sfx] * k
    for metric in ("lapvar", "tenengrad"):
        for ignore, mode in ((False, "none"), (True, "none"), (True, "fisheye_circle")):
            want = framescore.finish(st8, 2, 3, (0, 2), metric, False, ignore, mode)
            assert framescore.finish(st16, 2, 3, (0, 2), metric, False, ignore, mode, unit=257) == want
    got = framescore.finish(st16, 2, 3, (0, 2), "lapvar", False, False, "none", unit=257)
    assert got[3] == 700 / 6 / 255.0 and got[0] == pytest.approx(5000 / 6 - 36.0, rel=1e-12)
    # sums that are no multiple of the unit: the quotients, not truncations
    odd = dict(st16, sum_gray=st16["sum_gray"] + 100, sum_mag2=st16["sum_mag2"] + 30000)
    got = framescore.finish(odd, 2, 3, (0, 2), "tenengrad", False, False, "none", unit=257)
    assert got[3] == pytest.approx((700 + 100 / 257) / 6 / 255.0, rel=1e-15)
    assert got[0] == pytest.approx((9100 + 30000 / 257 ** 2) / 6, rel=1e-15)
    assert framescore.in_gray_levels(st16, 257)["n_valid"] == 5


def _identity_frames():
    rng = np.random.default_rng(16)
    out = [rng.integers(0, 256, size=(41, 57), dtype=np.uint8), rng.integers(200, 256, size=(30, 30), dtype=np.uint8)]
    edge = np.full((24, 24), 242, np.uint8)           # 242 * 257 = 62194 < 62259 <= 62451 = 243 * 257
    edge[::2, 1::3] = 243
    edge[5:9, 5:9] = 17
    return out + [edge]


@pytest.mark.parametrize("metric", framescore.METRICS)
@pytest.mark.parametrize("ignore,mode,crop", [(False, "none", 0.8), (True, "none", 1.0), (True, "fisheye_circle", 1.0)])
def test_frames_times_257_score_as_their_8_bit_frames(metric, ignore, mode, crop):
    """C == 1: g16 = 257 v, every sum is the 8-bit sum times the unit, so the tuples agree to double rounding of exact ratios."""
    for v in _identity_frames():
        v16 = v.astype(np.uint16) * 257
        st8 = fnp.frame_stats(v, *framescore.band_rows(v.shape[0], crop), mode == "fisheye_circle", ignore)
        st16 = fnp16.frame_stats(v16, *framescore.band_rows(v.shape[0], crop), mode == "fisheye_circle", ignore)
        assert (st16["n_highlight"], st16["n_valid"]) == (st8["n_highlight"], st8["n_valid"])
        want = fnp.score(v, metric, crop, True, ignore, mode)
        got = fnp16.score(v16, metric, crop, True, ignore, mode)
        # the fft term too: the float32 product (257 v) * float32(255 / 65535) is v itself for every v in 0..255
        assert np.array_equal(fnp16.fft_input(v16, 0, v.shape[0])[0], fnp.fft_input(v, 0, v.shape[0])[0])
        for k in range(9):
            assert (got[k] is None) == (want[k] is None)
            if got[k] is not None:
                assert got[k] == pytest.approx(want[k], rel=1e-12, abs=0.0), (k, metric)


def test_highlight_threshold_is_the_references():
    """62259 is the smallest g16 whose float32 gray, as the reference computes it, reaches 0.95 * 255."""
    g = np.arange(62000, 62600, dtype=np.uint16)
    ref = g.astype(np.float32) * fnp16.SCALE32 >= np.float32(0.95 * 255.0)
    assert np.array_equal(ref, g >= fnp16.HIGHLIGHT16) and framescore.HIGHLIGHT_LEVEL16 == fnp16.HIGHLIGHT16
    level = (g.astype(np.int64) + 192) // 257                      # plane 1 of the fft input
    assert np.array_equal(level >= framescore.HIGHLIGHT_LEVEL, ref)
    assert (65535 + 192) // 257 == 255


def _frames(seed):
    rng = np.random.default_rng(seed)
    out = []
    for H, W, C in [(67, 35, 1), (48, 90, 3), (130, 31, 4), (75, 120, 3)]:
        shape = (H, W) if C == 1 else (H, W, C)
        out.append(rng.integers(0, 65536, size=shape, dtype=np.uint16))
        yy, xx = np.mgrid[:H, :W]
        g = (xx * 1799 + yy * 771) % 65536
        g = np.where((xx - W / 3) ** 2 + (yy - H / 2) ** 2 < (min(H, W) / 4) ** 2, 64250, g)
        g = np.clip(g + rng.integers(-700, 701, size=g.shape), 0, 65535).astype(np.uint16)
        out.append(g if C == 1 else np.repeat(g[:, :, None], C, axis=2) ^ (np.arange(C, dtype=np.uint16) * 4369))
        ramp = ((xx * 40 + yy * 25) % 65536).astype(np.uint16)
        out.append(np.repeat(ramp[:, :, None], C, axis=2).reshape(shape))
    return out


def test_model_against_the_references_float32_chain():
    worst = 0.0
    for img in _frames(1):
        for metric in framescore.METRICS:
            for ignore, mode, crop in ((False, "none", 0.8), (True, "none", 1.0), (True, "fisheye_circle", 1.0),
                                       (False, "fisheye_circle", 0.6)):
                got = fnp16.score(img, metric, crop, True, ignore, mode)
                ref = fnp16.reference_f32(img, metric, crop, True, ignore, mode)
                assert got[2] == ref[2]                                   # p255: the highlight mask is the reference's exactly
                worst = max(worst, fnp16.largest_relative_difference(got, ref))
    print(f"largest relative difference from the float32 chain: {worst:.3e}")
    assert worst <= 4 * MEASURED_F32_DIFFERENCE
