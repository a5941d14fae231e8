"""NumPy restatement of MSK-SPEC v1, written from the definition: a dilate is, per element row, one OR of the
mask shifted over that row's span; an erode the AND of the same shifts with outside pixels counting as set; the strip fills are the
loops of SEG:473-495.  Nothing here follows the kernels' scheme (bit planes, windows, bands)."""
import numpy as np

from gs360 import maskfinish


def shifted(B, dy, dx, outside):
    """-> S with S[y, x] = B[y + dy, x + dx] inside the image and `outside` elsewhere"""
    H, W = B.shape
    S = np.full((H, W), outside, bool)
    ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
    if ys.start < ys.stop and xs.start < xs.stop:
        S[ys, xs] = B[ys.start + dy:ys.stop + dy, xs.start + dx:xs.stop + dx]
    return S


def row_or(B, dy, lo, hi):
    """OR over dx in [lo, hi] of shifted(B, dy, dx): one cumulative count along the row"""
    H, W = B.shape
    S = shifted(B, dy, 0, False)
    c = np.concatenate([np.zeros((H, 1), np.int64), np.cumsum(S, axis=1)], axis=1)
    x = np.arange(W)
    a, b = np.clip(x + lo, 0, W), np.clip(x + hi + 1, 0, W)
    return c[:, b] - c[:, a] > 0


def dilate(B, kw, kh):
    rows, (ax, ay) = maskfinish.structuring_rows(kw, kh)
    out = np.zeros(B.shape, bool)
    for i, (j1, j2) in enumerate(rows):
        if j2 > j1:
            out |= row_or(B, i - ay, j1 - ax, j2 - 1 - ax)
    return out


def erode(B, kw, kh):
    """the AND over the element's offsets, outside pixels set: what is left unset is what any unset inside pixel reaches"""
    rows, (ax, ay) = maskfinish.structuring_rows(kw, kh)
    hit = np.zeros(B.shape, bool)
    for i, (j1, j2) in enumerate(rows):
        if j2 > j1:
            hit |= row_or(~B, i - ay, j1 - ax, j2 - 1 - ax)
    return ~hit


def close(B, k):
    k = max(1, int(k))
    return erode(dilate(B, k, k), k, k) if k > 1 else B


def expand(B, p):
    return dilate(B, 2 * p + 1, 2 * p + 1) if p > 0 else B


def fuse(B, edge_fuse_pixels):
    """fuse_mask_to_edges (SEG:439-496) on a boolean mask"""
    f, s = maskfinish.fuse_spread(edge_fuse_pixels)
    if f <= 0 or not B.any():
        return B
    H, W = B.shape
    if f > min(H, W):
        raise ValueError("edge_fuse_pixels exceeds the mask's shorter side")
    out = B.copy()
    top, bottom = dilate(B[:f, :], 2 * s + 1, 1), dilate(B[H - f:, :], 2 * s + 1, 1)
    left, right = dilate(B[:, :f], 1, 2 * s + 1), dilate(B[:, W - f:], 1, 2 * s + 1)
    for x in np.where(top.any(axis=0))[0]:
        out[:np.where(top[:, x])[0].min() + 1, x] = True
    for x in np.where(bottom.any(axis=0))[0]:
        out[H - f + np.where(bottom[:, x])[0].max():, x] = True
    for y in np.where(left.any(axis=1))[0]:
        out[y, :np.where(left[y, :])[0].min() + 1] = True
    for y in np.where(right.any(axis=1))[0]:
        out[y, W - f + np.where(right[y, :])[0].max():] = True
    return out


def chain(raw, params, add=None, shape=None):
    """-> the finished boolean mask.  raw: H x W uint8 or None (no detection; shape = (H, W) then)"""
    B = np.zeros(shape, bool) if raw is None else np.asarray(raw) > params.thresh
    B = close(B, params.close)
    B = expand(B, maskfinish.resolve_expand_pixels(params.expand_mode, params.expand_pixels, params.expand_percent, B.shape))
    B = fuse(B, params.edge_fuse_pixels)
    if add is not None:
        B = B | (np.asarray(add) > 0)
    return B


def compose(B, kind, invert, image=None):
    """-> (the output array, the count) of step 6, with the empty-mask branches of SEG:742-781"""
    count = int(B.sum())
    m = np.where(B, 255, 0).astype(np.uint8)
    a = (255 - m) if invert else m
    if kind == "mask":
        return a, count
    if kind == "rgba":
        return np.dstack([image, a if count else np.zeros_like(a)]), count
    if not count:
        return image.copy(), count
    sel = B if kind == "keep" else ~B
    return np.where(sel[:, :, None], image, 0).astype(np.uint8), count


def finish(raw, params, add=None, image=None, kind="mask", invert=True, shape=None):
    return compose(chain(raw, params, add, shape), kind, invert, image)


def brute_morph(B, kw, kh, erode_):
    """four loops over the definition (small masks only)"""
    rows, (ax, ay) = maskfinish.structuring_rows(kw, kh)
    H, W = B.shape
    out = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            v = bool(erode_)
            for i, (j1, j2) in enumerate(rows):
                for j in range(j1, j2):
                    yy, xx = y + i - ay, x + j - ax
                    if 0 <= yy < H and 0 <= xx < W:
                        v = (v and B[yy, xx]) if erode_ else (v or B[yy, xx])
            out[y, x] = v
    return out


def brute_fuse(B, edge_fuse_pixels):
    """the edge fuse pixel by pixel from the spec's sentences (small masks only): no element, no dilate, no slices"""
    f, s = maskfinish.fuse_spread(edge_fuse_pixels)
    H, W = B.shape
    out = B.copy()
    if f <= 0:
        return out
    for y in range(H):
        for x in range(W):
            # the top strip fills above its topmost set row, the bottom strip below its lowest one; neither is spread
            top = [yy for yy in range(f) if B[yy, x]]
            bottom = [yy for yy in range(H - f, H) if B[yy, x]]
            # the side strips are spread s rows up and down first
            near = range(max(0, y - s), min(H, y + s + 1))
            left = [xx for xx in range(f) if any(B[yy, xx] for yy in near)]
            right = [xx for xx in range(W - f, W) if any(B[yy, xx] for yy in near)]
            if (top and y <= top[0]) or (bottom and y >= bottom[-1]) or (left and x <= left[0]) or (right and x >= right[-1]):
                out[y, x] = True
    return out
