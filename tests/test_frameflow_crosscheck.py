"""FS-FLOW v1 against the reference's own OpenCV calls (cv2.resize INTER_AREA, goodFeaturesToTrack, calcOpticalFlowPyrLK), where
cv2 is importable.  The spec differs from OpenCV only in float rounding (exact integer box and LK sums where OpenCV accumulates
in float) and in the gray of the decoded colour frame; these tests put a number on both."""
import math

import numpy as np
import pytest

import frameflow_np as fnp
from gs360 import frameflow

cv2 = pytest.importorskip("cv2")


def _blocks(rng, H, W, block=6):
    g = np.repeat(np.repeat(rng.integers(0, 256, (H // block + 2, W // block + 2)), block, 0), block, 1)
    return np.clip(g + rng.integers(-3, 4, g.shape), 0, 255).astype(np.uint8)


def _cv_value(a, b):
    p0 = cv2.goodFeaturesToTrack(a, maxCorners=1000, qualityLevel=0.01, minDistance=5, blockSize=7)
    if p0 is None:
        return None, None
    p1, st, _ = cv2.calcOpticalFlowPyrLK(a, b, p0, None, winSize=(15, 15), maxLevel=2,
                                         criteria=(cv2.TERM_CRITERIA_EPS | cv2.TERM_CRITERIA_COUNT, 10, 0.03))
    st = st.reshape(-1) == 1
    return float(np.mean(np.linalg.norm((p1[st] - p0[st]).reshape(-1, 2), axis=1))), p0.reshape(-1, 2)


@pytest.mark.parametrize("H, W, sw, sh", [(960, 1920, 320, 160), (3840, 3840, 320, 320), (700, 900, 320, 248)])
def test_inter_area_matches_cv2(H, W, sw, sh):
    rng = np.random.default_rng(H + W)
    g = rng.integers(0, 256, (H, W)).astype(np.uint8)
    fast = frameflow.area_fast_factors(W, H, sw, sh)
    mine = fnp.area_fast(g, *fast) if fast else fnp.area_general(g, sw, sh)
    ref = cv2.resize(g, (sw, sh), interpolation=cv2.INTER_AREA)
    assert np.abs(mine.astype(int) - ref.astype(int)).max() <= 1


def test_corners_and_values_match_cv2():
    rng = np.random.default_rng(1)
    big = _blocks(rng, 200, 360)
    a, b = big[20:180, 20:340], big[22:182, 17:337]
    ref, p0 = _cv_value(a, b)
    geom = frameflow.flow_geometry(160, 320, 1.0)
    fa = fnp.Frame(a, geom, False)
    mine = frameflow.value_of(fnp.pair(fa, fnp.Frame(b, geom, False))[0])
    common = {tuple(p) for p in p0.astype(int).tolist()} & {tuple(p) for p in fa.corners.astype(int).tolist()}
    assert len(common) >= 0.95 * len(p0)
    assert math.isclose(mine, ref, rel_tol=1e-2)
