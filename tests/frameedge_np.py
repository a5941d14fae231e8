"""NumPy restatement of FS-EDGE v1: the three integer sums of gs360_frame_edge_u8 and the 9-tuple the host
forms from them, written from the spec (not from the kernel) so that the GPU tests compare two readings of it.  A helper module of
the tests, not a test file."""
import numpy as np

from framescore_np import gray_u8

FIELDS = ("n", "sum_gray", "sum_edge")


def mirror(i, n):
    """The spec's tap coordinate: |i| inside [0, n), else 2n - 1 - |i| (-1 -> 1, n -> n - 1; n = 1 -> 0 everywhere)."""
    a = abs(i)
    return a if a < n else 2 * n - 1 - a


def isqrt_clip(s):
    """min(255, floor(sqrt(s))) per element of a non-negative int64 array, exact (math.isqrt's value): the float64 root is a
    candidate that integer compares settle."""
    s = np.asarray(s, np.int64)
    r = np.sqrt(s.astype(np.float64)).astype(np.int64)
    r -= r * r > s
    r += (r + 1) * (r + 1) <= s
    return np.minimum(r, 255)


def edge_image(band):
    """e of every pixel of an int64 image that stands on its own (the crop runs before the edge filter)."""
    h, w = band.shape
    ys = [mirror(i, h) for i in range(-1, h + 1)]
    xs = [mirror(i, w) for i in range(-1, w + 1)]
    p = band[np.array(ys)][:, np.array(xs)]

    def t(r, c):
        return p[r:r + h, c:c + w]
    ga = -t(0, 0) - 2 * t(0, 1) - t(0, 2) + t(2, 0) + 2 * t(2, 1) + t(2, 2)
    gb = -t(0, 0) + t(0, 2) - 2 * t(1, 0) + 2 * t(1, 2) - t(2, 0) + t(2, 2)
    return isqrt_clip(ga * ga + gb * gb)


def frame_edge(img, y0, y1, red_index=0):
    """-> dict of the gs360_frame_edge fields for one frame and band rows [y0, y1)."""
    band = gray_u8(img, red_index)[y0:y1]
    return {"n": int(band.size), "sum_gray": int(band.sum()), "sum_edge": int(edge_image(band).sum())}


def band(H, crop_ratio):
    """The filter graph's crop: only below 1.0; max(1, trunc(H * ratio)) rows at trunc((H - rows) / 2)."""
    if not crop_ratio < 1.0:
        return 0, H
    bh = max(1, int(H * crop_ratio))
    y0 = int((H - bh) / 2)
    return y0, y0 + bh


def score(img, crop_ratio, red_index=0):
    """The 9-tuple of score_one_file_ffmpeg from the restatement: YAVG through %g, then the reference's clamps and dark penalty."""
    H = np.asarray(img).shape[0]
    rec = frame_edge(img, *band(H, crop_ratio), red_index)
    y_gray = float("%g" % (rec["sum_gray"] / rec["n"]))
    y_edge = float("%g" % (rec["sum_edge"] / rec["n"]))
    bright = max(0.0, min(1.0, y_gray / 255.0))
    sharp = max(0.0, min(1.0, y_edge / 255.0))
    dark = bright / 0.35 if bright < 0.35 else 1.0
    dark = max(0.0, min(1.0, dark))
    return (sharp, 0.0, 0.0, bright, max(0.0, 1.0 - 0.5 * (1.0 - dark)), None, None, None, 1.0)
