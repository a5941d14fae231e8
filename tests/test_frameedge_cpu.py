"""FS-EDGE v1 on hand-derivable images: the NumPy restatement (tests/frameedge_np.py) and the host side of
gs360.framescore's default backend (the band, the %g quantisation of YAVG, the tuple).  No GPU."""
import math

import numpy as np
import pytest

import frameedge_np as enp
from gs360 import framescore


def _rec(img, y0=0, y1=None):
    img = np.asarray(img, np.uint8)
    return enp.frame_edge(img, y0, img.shape[0] if y1 is None else y1)


def test_mirror_is_not_reflect_101():
    assert [enp.mirror(i, 5) for i in (-1, 0, 4, 5)] == [1, 0, 4, 4]
    assert [enp.mirror(i, 1) for i in (-1, 0, 1)] == [0, 0, 0]
    assert [enp.mirror(i, 2) for i in (-1, 2)] == [1, 1]


def test_constant_image_has_no_edge():
    assert _rec(np.full((9, 13), 77)) == {"n": 117, "sum_gray": 77 * 117, "sum_edge": 0}


@pytest.mark.parametrize("d", [1, 10, 63, 64, 255])
def test_vertical_and_horizontal_steps(d):
    """A step of height d: the two columns (rows) at the step see |gb| (|ga|) = 4 d, every other pixel 0; d = 255 clips."""
    H, W = 12, 20
    img = np.zeros((H, W), np.uint8)
    img[:, 11:] = d
    e = min(255, 4 * d)
    assert _rec(img) == {"n": H * W, "sum_gray": d * H * 9, "sum_edge": 2 * H * e}
    assert np.array_equal(enp.edge_image(img.astype(np.int64))[:, 10:12], np.full((H, 2), e))
    assert _rec(img.T.copy()) == {"n": H * W, "sum_gray": d * H * 9, "sum_edge": 2 * H * e}


def test_ramp_reaching_the_last_column_and_row():
    """gray = 3x: inside gb = 8 * 3 = 24; at x = 0 both side taps are column 1 -> 0; at x = W-1 the right tap is column W-1
    itself (the mirror's len -> len-1) -> gb = 4 * 3 = 12, where reflect-101 (len -> len-2) gives 0."""
    H, W = 6, 10
    img = np.tile(3 * np.arange(W), (H, 1))
    assert _rec(img) == {"n": 60, "sum_gray": 3 * 45 * H, "sum_edge": H * (24 * (W - 2) + 12)}       # 1224; reflect-101: 1152
    assert _rec(img.T.copy()) == {"n": 60, "sum_gray": 3 * 45 * H, "sum_edge": H * (24 * (W - 2) + 12)}
    # both ramps at once, gray = 3x + 5y: inside (ga, gb) = (40, 24) -> 46; the corner (W-1, H-1) sees (20, 12) -> 23
    yy, xx = np.mgrid[:H, :W]
    e = enp.edge_image((3 * xx + 5 * yy).astype(np.int64))
    assert e[2, 3] == 46 and e[H - 1, W - 1] == 23 and e[0, 0] == 0
    assert e[H - 1, 3] == 31 and e[2, W - 1] == 41 and e[0, 3] == 24 and e[2, 0] == 40   # (20,24) (40,12) (0,24) (40,0)


def test_one_pixel_and_one_row_bands():
    assert _rec([[200]]) == {"n": 1, "sum_gray": 200, "sum_edge": 0}
    row = np.array([[0, 0, 10, 10, 10, 50]])
    # a 1 x N band: all three tap rows are the row itself, gb = 4 * (right - left), ga = 0
    assert _rec(row) == {"n": 6, "sum_gray": 80, "sum_edge": 0 + 40 + 40 + 0 + 160 + 160}
    img = np.zeros((5, 6), np.uint8)
    img[2] = row
    assert _rec(img, 2, 3) == _rec(row)             # the band is an image of its own: the rows around it do not count


def test_band_of_a_colour_frame_uses_the_spec_gray():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, size=(8, 9, 3), dtype=np.uint8)
    g = (img[..., 0].astype(np.int64) * 4899 + img[..., 1].astype(np.int64) * 9617 + img[..., 2].astype(np.int64) * 1868 + 8192) >> 14
    assert enp.frame_edge(img, 1, 7) == _rec(g, 1, 7)
    assert enp.frame_edge(img[..., ::-1].copy(), 1, 7, red_index=2) == _rec(g, 1, 7)


def test_integer_square_root_is_exact():
    s = np.array([0, 1, 3, 4, 24, 25, 65024, 65025, 2080800, 1442 ** 2 - 1])
    assert enp.isqrt_clip(s).tolist() == [0, 1, 1, 2, 4, 5, 254, 255, 255, 255]
    every = np.arange(0, 70000)
    assert enp.isqrt_clip(every).tolist() == [min(255, math.isqrt(int(v))) for v in every]


def test_yavg_is_quantised_like_percent_g():
    assert framescore.yavg(123456789, 1000000) == 123.457
    assert framescore.yavg(1, 3) == 0.333333
    assert framescore.yavg(510, 2) == 255.0


@pytest.mark.parametrize("H,crop,want", [(100, 0.8, (10, 90)), (37, 0.8, (4, 33)), (100, 1.0, (0, 100)), (100, 0.001, (49, 50)),
                                         (101, 0.001, (50, 51)), (3840, 0.8, (384, 3456)), (7, 1.5, (0, 7))])
def test_band_expression(H, crop, want):
    assert framescore.edge_band_rows(H, crop) == want == enp.band(H, crop)


def test_tuple_and_dark_penalty_on_both_sides_of_the_threshold():
    n = 1000
    dim = framescore.finish_edge({"n": n, "sum_gray": 51 * n, "sum_edge": 30 * n})        # 0.2 < 0.35
    assert dim == (30 / 255.0, 0.0, 0.0, 0.2, 1.0 - 0.5 * (1.0 - 0.2 / 0.35), None, None, None, 1.0)
    lit = framescore.finish_edge({"n": n, "sum_gray": 102 * n, "sum_edge": 255 * n})      # 0.4 >= 0.35
    assert lit == (1.0, 0.0, 0.0, 0.4, 1.0, None, None, None, 1.0)
    black = framescore.finish_edge({"n": n, "sum_gray": 0, "sum_edge": 0})
    assert black == (0.0, 0.0, 0.0, 0.0, 0.5, None, None, None, 1.0)


def test_restated_score_matches_the_host_finish():
    rng = np.random.default_rng(2)
    img = rng.integers(0, 90, size=(40, 50, 3), dtype=np.uint8)
    rec = enp.frame_edge(img, *enp.band(40, 0.8))
    assert framescore.finish_edge(rec) == enp.score(img, 0.8)
