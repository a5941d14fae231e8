"""NumPy restatement of FS-DEPTH16 v1, part 1: the statistics of gs360_frame_stats_u16 in int64, in units
of 1/257 gray level, and its fft input in float32; written from the spec, with the helpers of tests/framescore_np.py.  Also the
float32 restatement of the reference's own chain on a 16-bit image (FS:922-1036), which the exact model is measured against.
A helper module of the tests, not a test file."""
import math

import numpy as np

import framescore_np as fnp
from gs360 import framescore

HIGHLIGHT16 = 62259                   # the smallest g16 with g16 / 257 >= 0.95 * 255
SCALE32 = np.float32(255.0 / 65535.0)  # the reference's factor as its float32 array product takes it


def gray_u16(img, red_index=0):
    """H x W (x C) uint16 -> int64 g16: cv2 BGR2GRAY on 16U has the 8U coefficients; alpha ignored."""
    assert np.asarray(img).dtype == np.uint16
    return fnp.gray_u8(img, red_index)     # the formula is written on int64 copies of the samples


def view8(img):
    """The 8-bit view the edge and flow passes read: every sample >> 8."""
    return (np.asarray(img) >> 8).astype(np.uint8)


def frame_stats(img, y0, y1, circle_on=False, highlights_on=False, red_index=0):
    """-> dict of the gs360_frame_stats fields of one 16-bit frame (sums in units of 1/257, and of 1/257^2 for the squares)."""
    g = gray_u16(img, red_index)
    H, W = g.shape
    circ = fnp.circle(H, W)
    hl = g >= HIGHLIGHT16
    band = g[y0:y1]
    lap, gx, gy = fnp.laplacian_sobel(band)
    mag2 = gx * gx + gy * gy
    valid = np.ones(band.shape, bool)
    if circle_on:
        valid &= circ[y0:y1]
    if highlights_on:
        valid &= ~hl[y0:y1]
    st = {"n_circle": int(circ.sum()), "n_highlight": int(hl.sum()), "n_highlight_in_circle": int((hl & circ).sum())}
    for sfx, m in (("", np.ones(band.shape, bool)), ("_valid", valid)):
        st["n" + sfx] = int(m.sum())
        st["sum_gray" + sfx] = int(band[m].sum())
        st["sum_lap" + sfx] = int(lap[m].sum())
        st["sum_lap2" + sfx] = int((lap[m] * lap[m]).sum())        # |lap| <= 8 * 65535: a square is < 2^39, int64 holds the sum
        st["sum_mag2" + sfx] = int(mag2[m].sum())
    return st


def fft_input(img, y0, y1, red_index=0):
    """(plane 0, plane 1) as the kernel writes them: INTER_AREA of the float32 products g16 * float32(255 / 65535), and the level
    floor(g16 / 257 + 0.75) at the nearest sample (>= 243 exactly when g16 >= 62259)."""
    g16 = gray_u16(img, red_index)[y0:y1]
    g = g16.astype(np.float32) * SCALE32
    bh, bw = g.shape
    nw, nh = framescore.fft_input_size(bw, bh)
    iy, ix = framescore.nearest_index(nh, bh), framescore.nearest_index(nw, bw)
    level = ((g16 + 192) // 257).astype(np.float32)
    return fnp.inter_area(g, nw, nh), level[iy][:, ix]


def score(img, metric, crop_ratio, augment_motion, ignore_highlights, mask_mode="none", red_index=0):
    """The 9-tuple from the exact model: framescore.finish(unit=257) on the restated statistics."""
    a = np.asarray(img)
    H, W = a.shape[:2]
    y0, y1 = framescore.band_rows(H, crop_ratio)
    st = frame_stats(a, y0, y1, mask_mode == "fisheye_circle", bool(ignore_highlights), red_index)
    small = fft_input(a, y0, y1, red_index) if metric in ("fft", "hybrid") else None
    return framescore.finish(st, H, W, (y0, y1), metric, augment_motion, ignore_highlights, mask_mode, small, unit=257)


# ---- the reference's float32 chain -------------------------------------------------------------------------------------------
def _mean_std2(values):
    """cv2.meanStdDev on float32 values: double sums, std^2 = max(sq / n - mean^2, 0)."""
    v = values.astype(np.float64)
    mean = v.sum() / v.size
    return max((v * v).sum() / v.size - mean * mean, 0.0)


def reference_f32(img, metric, crop_ratio, augment_motion, ignore_highlights, mask_mode="none", red_index=0):
    """score_one_file (FS:922-1036) on a 16-bit image, restated in NumPy from `gray = g16.astype(float32) * (255 / 65535)` onward:
    float32 gray, float32 Laplacian / Sobel responses and squares, double accumulation where cv2 accumulates in double."""
    g16 = gray_u16(img, red_index)
    H, W = g16.shape
    gray = np.clip(g16.astype(np.float32) * SCALE32, np.float32(0.0), np.float32(255.0))
    valid = fnp.circle(H, W) if mask_mode == "fisheye_circle" else None
    p255 = 0.0
    if ignore_highlights:
        hl = gray >= np.float32(0.95 * 255.0)         # 242.25 is a float32
        if valid is not None and valid.any():
            p255 = float(np.count_nonzero(hl & valid) / float(np.count_nonzero(valid)))
        else:
            p255 = float(np.mean(hl))
        if valid is None:
            if 0.0 < p255 < 1.0:
                valid = ~hl
        else:
            valid = valid & ~hl
    y0, y1 = framescore.band_rows(H, crop_ratio)
    gray = gray[y0:y1]
    valid = None if valid is None else valid[y0:y1]
    use = valid is not None and valid.any()
    sel = valid if use else np.ones(gray.shape, bool)
    brightness_mean = float(gray[sel].astype(np.float64).sum() / sel.sum() / 255.0) if use else float(float(np.mean(gray)) / 255.0)
    p = np.pad(gray, 1, mode="reflect")
    bh, bw = gray.shape

    def at(dy, dx):
        return p[1 + dy:1 + dy + bh, 1 + dx:1 + dx + bw]
    two, eight = np.float32(2.0), np.float32(8.0)
    lap = two * at(-1, -1) + two * at(-1, 1) - eight * at(0, 0) + two * at(1, -1) + two * at(1, 1)      # float32, row-major taps
    gx = (at(-1, 1) - at(-1, -1)) + two * (at(0, 1) - at(0, -1)) + (at(1, 1) - at(1, -1))
    gy = (at(1, -1) - at(-1, -1)) + two * (at(1, 0) - at(-1, 0)) + (at(1, 1) - at(-1, 1))
    mag2 = gx * gx + gy * gy                                                                            # float32
    lap_score = _mean_std2(lap[sel]) if metric in ("lapvar", "hybrid") else None
    ten_score = float(mag2[sel].astype(np.float64).sum() / sel.sum()) if metric in ("tenengrad", "hybrid") else None
    fft_score = None
    if metric in ("fft", "hybrid"):
        nw, nh = framescore.fft_input_size(bw, bh)
        small = fnp.inter_area(gray, nw, nh)
        g_mask = None
        if use:
            iy, ix = framescore.nearest_index(nh, bh), framescore.nearest_index(nw, bw)
            g_mask = valid[iy][:, ix].astype(np.uint8)
        fft_score = framescore.fft_energy(small, g_mask)
    brightness_weight, motion_factor = 1.0, 1.0
    lap_feature = ten_feature = fft_feature = None
    if metric == "lapvar":
        sharp, lap_feature = lap_score, lap_score * lap_score
    elif metric == "tenengrad":
        sharp = ten_feature = ten_score
    elif metric == "fft":
        sharp = fft_feature = fft_score
    else:
        lap_feature, ten_feature, fft_feature = lap_score * lap_score, ten_score, fft_score
        raw = (framescore.HYBRID_LAPVAR_WEIGHT * lap_feature + framescore.HYBRID_TENENGRAD_WEIGHT * ten_score
               + framescore.HYBRID_FFT_WEIGHT * fft_score)
        if augment_motion:
            ratio = max(0.0, min(1.0, ten_score / (ten_score + framescore.HYBRID_MOTION_REFERENCE)))
            motion_factor = max(0.0, 1.0 - framescore.HYBRID_MOTION_PENALTY_WEIGHT * (1.0 - ratio))
        dark = brightness_mean / framescore.HYBRID_DARK_THRESHOLD if brightness_mean < framescore.HYBRID_DARK_THRESHOLD else 1.0
        dark = max(0.0, min(1.0, dark))
        brightness_weight = max(0.0, 1.0 - framescore.HYBRID_DARK_PENALTY_WEIGHT * (1.0 - dark))
        sharp = raw * motion_factor
    return (sharp, 0.0, p255, brightness_mean, brightness_weight, lap_feature, ten_feature, fft_feature, motion_factor)


def largest_relative_difference(a, b):
    """max over the fields both tuples hold as numbers of |a - b| / max(|a|, |b|) (0 where both are 0); None fields must agree."""
    worst = 0.0
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is None or x == y:
            continue
        assert math.isfinite(x) and math.isfinite(y)
        worst = max(worst, abs(x - y) / max(abs(x), abs(y)))
    return worst
