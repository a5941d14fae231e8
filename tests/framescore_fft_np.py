"""NumPy restatement of FS-FFT v1: the gs360_frame_fft record of one frame from its two fft-input planes, the frame
geometry and the flags, in float64 -- written from the spec, not from the kernel.  half_spectrum_record restates the kernel's
decomposition (the w/2+1 Hermitian columns, each credited at its own and its mirrored fftshift position) so that the crediting
rule is checked without a GPU.  A helper module of the tests, not a test file."""
import numpy as np

from gs360 import capi, framescore


def geometry(h, w, H, W, band, flags, g_near):
    """(donut, valid) boolean h x w images at the shifted / spatial positions (i, j)."""
    cy, cx = h // 2, w // 2
    r = max(1, min(h, w) // 8)
    yy, xx = np.ogrid[:h, :w]
    donut = (yy - cy) ** 2 + (xx - cx) ** 2 >= r * r
    valid = np.ones((h, w), bool)
    if flags & capi.FS_CIRCLE:
        y0, y1 = band
        ys = y0 + framescore.nearest_index(h, y1 - y0)
        xs = framescore.nearest_index(w, W)
        valid &= framescore.circle_mask(H, W, ys, xs)
    if flags & capi.FS_HIGHLIGHTS:
        valid &= np.asarray(g_near) < framescore.HIGHLIGHT_LEVEL
    return donut, valid


def fft_record(g, g_near, H, W, band, flags):
    """-> dict of the gs360_frame_fft fields: |fftshift(fft2(g))| summed over the donut and over donut & valid, in float64."""
    g = np.asarray(g, np.float64)
    h, w = g.shape
    mag = np.abs(np.fft.fftshift(np.fft.fft2(g)))
    donut, valid = geometry(h, w, H, W, band, flags, g_near)
    return {"sum_hf": float(mag[donut].sum()), "sum_hf_valid": float(mag[donut & valid].sum()), "n_valid": int(valid.sum()),
            "n": h * w}


def half_spectrum_record(g, g_near, H, W, band, flags):
    """The same record from the columns k = 0 .. w/2 of the spectrum only: |F(u, k)| credited at the shifted position of (u, k)
    and, except for k = 0 and (even w) k = w/2, at that of (-u, -k)."""
    g = np.asarray(g, np.float64)
    h, w = g.shape
    K = w // 2 + 1
    mag = np.abs(np.fft.fft(np.fft.fft(g, axis=1)[:, :K], axis=0))
    donut, valid = geometry(h, w, H, W, band, flags, g_near)
    acc = np.zeros((h, w))
    hits = np.zeros((h, w), np.int64)
    u = np.arange(h)[:, None]
    for k in range(K):
        pos = [(u[:, 0], k)]
        if k != 0 and 2 * k != w:
            pos.append(((-u[:, 0]) % h, w - k))
        for uu, kk in pos:
            i, j = (uu + h // 2) % h, (kk + w // 2) % w
            acc[i, j] += mag[:, k]
            hits[i, j] += 1
    assert (hits == 1).all(), "every shifted position is credited exactly once"
    return {"sum_hf": float(acc[donut].sum()), "sum_hf_valid": float(acc[donut & valid].sum()), "n_valid": int(valid.sum()),
            "n": h * w}


def host_mask(g_near, H, W, band, mask_mode, ignore_highlights):
    """The resized mask finish() builds on the host when the statistics say `masked` (as uint8, or None)."""
    h, w = np.asarray(g_near).shape
    flags = (capi.FS_CIRCLE if mask_mode == "fisheye_circle" else 0) | (capi.FS_HIGHLIGHTS if ignore_highlights else 0)
    return geometry(h, w, H, W, band, flags, g_near)[1].astype(np.uint8)
