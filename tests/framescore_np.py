"""NumPy restatement of FS-SPEC v1: the frame statistics of gs360_frame_stats_u8 in int64 and the INTER_AREA /
INTER_NEAREST fft input in float32, written from the spec (not from the kernel) so that the GPU tests compare two readings of it.
A helper module of the tests, not a test file."""
import numpy as np

from gs360 import framescore

FIELDS = framescore.FIELDS


def gray_u8(img, red_index=0):
    """H x W (x C) uint8 -> int64 gray: cv2 BGR2GRAY on 8U, (R*4899 + G*9617 + B*1868 + 8192) >> 14; alpha ignored."""
    a = np.asarray(img)
    if a.ndim == 2 or a.shape[2] == 1:
        return a.reshape(a.shape[0], a.shape[1]).astype(np.int64)
    r = a[:, :, red_index].astype(np.int64)
    g = a[:, :, 1].astype(np.int64)
    b = a[:, :, 2 - red_index].astype(np.int64)
    return (r * 4899 + g * 9617 + b * 1868 + 8192) >> 14


def circle(H, W):
    yy, xx = np.ogrid[:H, :W]
    return (2 * xx - (W - 1)) ** 2 + (2 * yy - (H - 1)) ** 2 <= max(4, min(W, H) ** 2)


def laplacian_sobel(band):
    """ksize-3 Laplacian [[2,0,2],[0,-8,0],[2,0,2]] and Sobel gx / gy of an int64 image, BORDER_REFLECT_101 at every edge
    (NumPy's 'reflect' padding is reflect-101)."""
    p = np.pad(band, 1, mode="reflect")
    h, w = band.shape

    def at(dy, dx):
        return p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    lap = 2 * (at(-1, -1) + at(-1, 1) + at(1, -1) + at(1, 1)) - 8 * at(0, 0)
    gx = (at(-1, 1) + 2 * at(0, 1) + at(1, 1)) - (at(-1, -1) + 2 * at(0, -1) + at(1, -1))
    gy = (at(1, -1) + 2 * at(1, 0) + at(1, 1)) - (at(-1, -1) + 2 * at(-1, 0) + at(-1, 1))
    return lap, gx, gy


def frame_stats(img, y0, y1, circle_on=False, highlights_on=False, red_index=0):
    """-> dict of the gs360_frame_stats fields for one frame."""
    g = gray_u8(img, red_index)
    H, W = g.shape
    circ = circle(H, W)
    hl = g >= 243
    band = g[y0:y1]
    lap, gx, gy = laplacian_sobel(band)
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
        st["sum_lap2" + sfx] = int((lap[m] * lap[m]).sum())
        st["sum_mag2" + sfx] = int(mag2[m].sum())
    return st


def area_tab(ssize, dsize):
    """cv::computeResizeAreaTab with cv::resize's scale = 1 / (dsize / ssize): per destination index the ordered list of
    (source index, float32 weight)."""
    scale = 1.0 / (float(dsize) / float(ssize))
    tab = []
    for d in range(dsize):
        f1 = d * scale
        f2 = f1 + scale
        cell = min(scale, ssize - f1)
        s1, s2 = int(np.ceil(f1)), int(np.floor(f2))
        s2 = min(s2, ssize - 1)
        s1 = min(s1, s2)
        e = []
        if s1 - f1 > 1e-3:
            e.append((s1 - 1, np.float32((s1 - f1) / cell)))
        e += [(s, np.float32(1.0 / cell)) for s in range(s1, s2)]
        if f2 - s2 > 1e-3:
            e.append((s2, np.float32(min(min(f2 - s2, 1.0), cell) / cell)))
        tab.append(e)
    return tab


def _apply_tab(tab, src, axis):
    """out[d] = sum over tab[d] of src[s] * w, float32, accumulated in the table's order (along `axis`)."""
    n_out = len(tab)
    shape = list(src.shape)
    shape[axis] = n_out
    out = np.zeros(shape, np.float32)
    depth = max(len(e) for e in tab)
    for p in range(depth):
        ds = np.array([d for d in range(n_out) if len(tab[d]) > p], np.int64)
        ss = np.array([tab[d][p][0] for d in ds], np.int64)
        ws = np.array([tab[d][p][1] for d in ds], np.float32)
        if axis == 1:
            out[:, ds] = out[:, ds] + src[:, ss] * ws[None, :]
        else:
            out[ds, :] = out[ds, :] + ws[:, None] * src[ss, :]
    return out


def inter_area(band_gray, nw, nh):
    """cv2.resize(band (float32), (nw, nh), INTER_AREA) through the general per-axis area path: each source row is reduced
    along x (buf += S * alpha), then rows are blended (sum += beta * buf), both in float32 and in table order."""
    src = np.asarray(band_gray, np.float32)
    bh, bw = src.shape
    rows = _apply_tab(area_tab(bw, nw), src, axis=1)
    return _apply_tab(area_tab(bh, nh), rows, axis=0)


def fft_input(img, y0, y1, red_index=0):
    """(area image, gray at the nearest sample) the kernel writes: the band itself when its long side is <= 512."""
    g = gray_u8(img, red_index)[y0:y1].astype(np.float32)
    bh, bw = g.shape
    nw, nh = framescore.fft_input_size(bw, bh)
    iy, ix = framescore.nearest_index(nh, bh), framescore.nearest_index(nw, bw)
    return inter_area(g, nw, nh), g[iy][:, ix]


def score(img, metric, crop_ratio, augment_motion, ignore_highlights, mask_mode="none", red_index=0):
    """The 9-tuple of score_one_file from the restatement (framescore.finish on restated statistics)."""
    a = np.asarray(img)
    H, W = a.shape[:2]
    y0, y1 = framescore.band_rows(H, crop_ratio)
    st = frame_stats(a, y0, y1, mask_mode == "fisheye_circle", bool(ignore_highlights), red_index)
    small = fft_input(a, y0, y1, red_index) if metric in ("fft", "hybrid") else None
    return framescore.finish(st, H, W, (y0, y1), metric, augment_motion, ignore_highlights, mask_mode, small)
