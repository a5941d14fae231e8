"""MSK-SPEC v1 against the reference's own OpenCV calls (cv2.getStructuringElement, cv2.dilate, cv2.morphologyEx), where cv2 is
importable.  structuring_rows restates OpenCV's ellipse from its source; until this file has run somewhere with cv2, parity of the
element (and with it of every step) with cv2 is unpinned.  No tolerance: the arithmetic is integer on both sides."""
import numpy as np
import pytest

from gs360 import maskfinish

import maskfinish_cases as cases
import maskfinish_np as ref

cv2 = pytest.importorskip("cv2")

CASES = {**cases.cases(), **cases.limit_cases()}        # the limit fixtures: a 1025 x 1025 ellipse, strips 200 wide


def fixture_elements():
    """every (kw, kh) a fixture's chain builds"""
    out = set()
    for c in CASES.values():
        H, W = cases.shape_of(c)
        k = max(1, int(c.params.close))
        p = maskfinish.resolve_expand_pixels(c.params.expand_mode, c.params.expand_pixels, c.params.expand_percent, (H, W))
        _f, s = maskfinish.fuse_spread(c.params.edge_fuse_pixels)
        out |= {(k, k), (2 * p + 1, 2 * p + 1), (2 * s + 1, 1), (1, 2 * s + 1)}
    return sorted(out)


def element(kw, kh):
    e = np.zeros((kh, kw), np.uint8)
    for i, (j1, j2) in enumerate(maskfinish.structuring_rows(kw, kh)[0]):
        e[i, j1:j2] = 1
    return e


def test_structuring_rows_is_cv2s_ellipse():
    for kw, kh in fixture_elements() + [(155, 155), (1025, 1025), (6, 4), (4, 6)]:
        assert np.array_equal(element(kw, kh), cv2.getStructuringElement(cv2.MORPH_ELLIPSE, (kw, kh))), (kw, kh)


def u8(B):
    return np.where(B, 255, 0).astype(np.uint8)


def test_each_step_equals_cv2():
    for name, c in CASES.items():
        shape = cases.shape_of(c)
        B = np.zeros(shape, bool) if c.raw is None else c.raw > c.params.thresh
        k = max(1, int(c.params.close))
        if k > 1:
            kernel = cv2.getStructuringElement(cv2.MORPH_ELLIPSE, (k, k))
            assert np.array_equal(u8(ref.dilate(B, k, k)), cv2.dilate(u8(B), kernel)), (name, "dilate")
            assert np.array_equal(u8(ref.erode(B, k, k)), cv2.erode(u8(B), kernel)), (name, "erode")
            assert np.array_equal(u8(ref.close(B, k)), cv2.morphologyEx(u8(B), cv2.MORPH_CLOSE, kernel)), (name, "close")
        p = maskfinish.resolve_expand_pixels(c.params.expand_mode, c.params.expand_pixels, c.params.expand_percent, shape)
        if p > 0:
            kernel = cv2.getStructuringElement(cv2.MORPH_ELLIPSE, (2 * p + 1, 2 * p + 1))
            assert np.array_equal(u8(ref.expand(B, p)), cv2.dilate(u8(B), kernel, iterations=1)), (name, "expand")
        f, s = maskfinish.fuse_spread(c.params.edge_fuse_pixels)
        if f > 0:
            for strip, (kw, kh) in ((B[:f, :], (2 * s + 1, 1)), (B[:, :f], (1, 2 * s + 1))):
                kernel = cv2.getStructuringElement(cv2.MORPH_ELLIPSE, (kw, kh))
                assert np.array_equal(u8(ref.dilate(strip, kw, kh)), cv2.dilate(u8(np.ascontiguousarray(strip)), kernel)), (name, "seed")
