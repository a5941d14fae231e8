"""MSK-SHADOW v1 against the cv2 calls it restates, step by step: GaussianBlur on a float plane, the S channel of cvtColor's 8-bit
RGB2HSV, and findContours(RETR_EXTERNAL) / contourArea / drawContours on the labelling fixtures.  The spec was written from OpenCV's
documented behaviour on machines without cv2 ("parity with cv2 unpinned"): this test pins it wherever cv2 is
installed, and skips elsewhere."""
import numpy as np
import pytest

from gs360 import maskfinish

import maskshadow_cases as cases
import maskshadow_np as ref

cv2 = pytest.importorskip("cv2")


BLUR = {**cases.blur_cases(), **cases.blur_limit_cases()}       # the limit fixtures: 511 taps, a row of 2100


@pytest.mark.parametrize("name", list(BLUR))
def test_gaussian_blur(name):
    c = BLUR[name]
    g = ref.gray_of(c.img).astype(np.float32)
    assert np.array_equal(ref.gray_of(c.img), cv2.cvtColor(c.img, cv2.COLOR_RGB2GRAY))
    w = maskfinish.gaussian_weights(c.sigma)
    assert np.array_equal(w, cv2.getGaussianKernel(len(w), c.sigma, cv2.CV_32F).ravel())
    assert np.array_equal(ref.blur(g, w[len(w) // 2:]), cv2.GaussianBlur(g, (0, 0), c.sigma))


def test_hsv_saturation():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    img[0, :16] = [(v, v, v) for v in range(0, 256, 16)]
    assert np.array_equal(ref.saturation(img), cv2.cvtColor(img, cv2.COLOR_RGB2HSV)[:, :, 1])


@pytest.mark.parametrize("size", cases.LABEL_SIZES + [cases.LABEL_WIDE])
@pytest.mark.parametrize("name", cases.LABEL_NAMES)
def test_the_contour_filter(size, name):
    X = cases.label_planes(*size)[name]
    shadow = np.where(X, 255, 0).astype(np.uint8)
    cnts, _ = cv2.findContours(shadow, cv2.RETR_EXTERNAL, cv2.CHAIN_APPROX_SIMPLE)
    clean = np.zeros_like(shadow)
    for c in cnts:
        if cv2.contourArea(c) >= cases.LABEL_MIN_AREA:
            cv2.drawContours(clean, [c], -1, 255, -1)
    _G, mine, areas = ref.component_filter(X, cases.LABEL_MIN_AREA)
    assert sorted(int(round(2 * cv2.contourArea(c))) for c in cnts) == areas
    assert np.array_equal(clean > 0, mine)
