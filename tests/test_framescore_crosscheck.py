"""FS-SPEC v1 against OpenCV itself, where cv2 is importable: the gray constants, the ksize-3 Laplacian / Sobel with
BORDER_REFLECT_101 on the band as an image of its own, meanStdDev / mean on the exact sums, and the INTER_AREA / INTER_NEAREST
fft input.  cv2 is not installed in the build or GPU images, so this SKIPS there; on the first box that has it, the restatement
(tests/framescore_np.py) becomes a measured fact."""
import numpy as np
import pytest

import framescore_np as fnp
from gs360 import framescore

cv2 = pytest.importorskip("cv2")


def _reference_stats(img_bgr, crop, circle, ignore_highlights):
    """score_one_file's masks, crop and lapvar32 / tenengrad32 / brightness (FS:902-990), through cv2."""
    gray = cv2.cvtColor(img_bgr, cv2.COLOR_BGR2GRAY).astype(np.float32) if img_bgr.ndim == 3 else img_bgr.astype(np.float32)
    H, W = gray.shape
    valid = fnp.circle(H, W).astype(np.uint8) if circle else None
    hl = gray >= 0.95 * 255.0
    if ignore_highlights:
        valid = (~hl).astype(np.uint8) if valid is None else ((valid > 0) & ~hl).astype(np.uint8)
    y0, y1 = framescore.band_rows(H, crop)
    g = gray[y0:y1]
    m = None if valid is None else valid[y0:y1]
    lap = cv2.Laplacian(g, cv2.CV_32F, ksize=3)
    gx = cv2.Sobel(g, cv2.CV_32F, 1, 0, ksize=3)
    gy = cv2.Sobel(g, cv2.CV_32F, 0, 1, ksize=3)
    mag2 = cv2.multiply(gx, gx) + cv2.multiply(gy, gy)
    mk = None if m is None or not np.any(m) else (m > 0).astype(np.uint8) * 255
    _, std = cv2.meanStdDev(lap, mask=mk)
    return (float(std[0, 0] * std[0, 0]), float(cv2.mean(mag2, mask=mk)[0]), float(cv2.mean(g, mask=mk)[0] / 255.0), g, (y0, y1))


@pytest.mark.parametrize("H,W,crop,circle,hl", [(120, 200, 0.8, False, False), (97, 131, 0.6, True, True), (64, 64, 1.0, True, False)])
def test_restatement_matches_opencv(H, W, crop, circle, hl):
    rng = np.random.default_rng(H + W)
    rgb = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    rgb[: H // 3, : W // 3] = 250
    bgr = np.ascontiguousarray(rgb[:, :, ::-1])
    lapvar, ten, bright, g, band = _reference_stats(bgr, crop, circle, hl)
    assert np.array_equal(fnp.gray_u8(rgb, 0), cv2.cvtColor(bgr, cv2.COLOR_BGR2GRAY))
    lap, gx, gy = fnp.laplacian_sobel(g.astype(np.int64))
    assert np.array_equal(lap, cv2.Laplacian(g, cv2.CV_32F, ksize=3))
    assert np.array_equal(gx * gx + gy * gy, cv2.Sobel(g, cv2.CV_32F, 1, 0, ksize=3) ** 2 + cv2.Sobel(g, cv2.CV_32F, 0, 1, ksize=3) ** 2)
    st = fnp.frame_stats(rgb, *band, circle, hl)
    got = framescore.finish(st, H, W, band, "hybrid", False, hl, "fisheye_circle" if circle else "none",
                            fnp.fft_input(rgb, *band))
    assert got[5] == lapvar * lapvar and got[6] == ten
    if circle or (hl and 0 < got[2] < 1):
        assert got[3] == bright                      # the masked brightness is cv2.mean: exact
    else:
        assert got[3] == pytest.approx(bright, rel=1e-6)   # np.mean in float32 (documented deviation)


@pytest.mark.parametrize("bh,bw", [(3072, 7680), (410, 1000), (600, 513), (64, 1024)])
def test_inter_area_and_nearest_match_opencv(bh, bw):
    rng = np.random.default_rng(bh)
    g = rng.integers(0, 256, size=(bh, bw)).astype(np.float32)
    nw, nh = framescore.fft_input_size(bw, bh)
    np.testing.assert_allclose(fnp.inter_area(g, nw, nh), cv2.resize(g, (nw, nh), interpolation=cv2.INTER_AREA), rtol=1e-5)
    near = g[framescore.nearest_index(nh, bh)][:, framescore.nearest_index(nw, bw)]
    assert np.array_equal(near, cv2.resize(g, (nw, nh), interpolation=cv2.INTER_NEAREST))
