"""NumPy restatement of MSK-SHADOW v1, written from the definition: the filter one tap at a time over index
maps that reflect as the spec's loop does, the saturation from the divisor table, the morphology as tests/maskfinish_np.py states it,
the component filter as two plain flood fills and a count over 2 x 2 cells.  Nothing here follows the kernels' scheme (staged tiles,
sliding windows, label equivalence)."""
import numpy as np

from gs360 import maskfinish

import maskfinish_np as mk


def reflect101(p, n):
    """BORDER_REFLECT_101 as borderInterpolate does it: a side of 1 maps everything to 0; otherwise p = -p below 0 and
    p = 2 (n - 1) - p from n on, repeated until inside"""
    p = np.array(p, np.int64)
    if n == 1:
        return np.zeros_like(p)
    while ((p < 0) | (p >= n)).any():
        p = np.where(p < 0, -p, p)
        p = np.where(p >= n, 2 * (n - 1) - p, p)
    return p


def gray_of(img):
    r, g, b = (img[:, :, c].astype(np.int64) for c in range(3))
    return ((4899 * r + 9617 * g + 1868 * b + 8192) >> 14).astype(np.uint8)


def filter_axis(v, half, axis):
    """s = k[0] v(c); s = s + k[i] (v(c - i) + v(c + i)), float32, every operation rounded on its own"""
    v = np.asarray(v, np.float32)
    n = v.shape[axis]
    at = np.arange(n)
    s = np.float32(half[0]) * v
    for i in range(1, len(half)):
        pair = np.take(v, reflect101(at - i, n), axis) + np.take(v, reflect101(at + i, n), axis)
        s = s + np.float32(half[i]) * pair
    assert s.dtype == np.float32
    return s


def blur(g, half):
    """rows, then columns; half = k[0 .. r], centre outward"""
    return filter_axis(filter_axis(np.asarray(g, np.float32), half, 1), half, 0)


def saturation(img, sdiv=None):
    sdiv = maskfinish.sat_div_table() if sdiv is None else sdiv
    v, lo = img.max(axis=2).astype(np.int64), img.min(axis=2).astype(np.int64)
    return ((v - lo) * sdiv[v].astype(np.int64) + 2048) >> 12


def candidates(img, half, t, delta_min, sat_max, sdiv=None):
    """step 3 -> C0"""
    g = gray_of(img).astype(np.float32)
    illum = blur(g, half)
    ratio = g / (illum + np.float32(1e-6))
    delta = illum - g
    assert ratio.dtype == np.float32 and delta.dtype == np.float32
    return (ratio < np.float32(t)) & (delta >= np.float32(delta_min)) & (saturation(img, sdiv) <= int(sat_max))


def dilate_rows(B, rows, kw, kh):
    out = np.zeros(B.shape, bool)
    for i, (j1, j2) in enumerate(rows):
        if j2 > j1 and abs(i - kh // 2) < B.shape[0]:    # (a row further away reads outside pixels only)
            out |= mk.row_or(B, i - kh // 2, j1 - kw // 2, j2 - 1 - kw // 2)
    return out


def erode_rows(B, rows, kw, kh):
    return ~dilate_rows(~B, rows, kw, kh)


def ellipse(k):
    return maskfinish.structuring_rows(k, k)[0], k, k


def flood(free, seeds, conn):
    """-> the pixels of `free` reached from the seeds over 4- or 8-neighbour steps (a plain fill over a one-pixel clear frame)"""
    H, W = free.shape
    Wp = W + 2
    ok = bytearray(np.pad(free, 1).astype(np.uint8).tobytes())         # reached pixels are cleared as they are queued
    steps = [-Wp, Wp, -1, 1] + ([-Wp - 1, -Wp + 1, Wp - 1, Wp + 1] if conn == 8 else [])
    todo = []
    for y, x in seeds:
        p = (y + 1) * Wp + x + 1
        if ok[p]:
            ok[p] = 0
            todo.append(p)
    at = 0
    while at < len(todo):
        p = todo[at]
        at += 1
        for d in steps:
            if ok[p + d]:
                ok[p + d] = 0
                todo.append(p + d)
    seen = np.zeros((H + 2) * Wp, bool)
    seen[todo] = True
    return seen.reshape(H + 2, Wp)[1:-1, 1:-1]


def outer_filled(C):
    """G: everything but the background that is 4-connected to a background pixel on the image border"""
    H, W = C.shape
    border = [(y, x) for y in range(H) for x in (0, W - 1)] + [(y, x) for x in range(W) for y in (0, H - 1)]
    return ~flood(~C, border, 4)


def components(G):
    """-> (labels: 0 outside G, 1 .. n per 8-connected component; n)"""
    labels = np.zeros(G.shape, np.int64)
    n = 0
    for y, x in zip(*np.nonzero(G)):
        if not labels[y, x]:
            n += 1
            labels[flood(G, [(y, x)], 8)] = n
    return labels, n


def doubled_areas(G, labels, n):
    """-> 2A per label (index 0 unused): 2 per cell with four corners in G, 1 per cell with three"""
    area2 = np.zeros(n + 1, np.int64)
    if min(G.shape) < 2:
        return area2
    corners = [G[:-1, :-1], G[:-1, 1:], G[1:, :-1], G[1:, 1:]]
    cnt = sum(c.astype(np.int64) for c in corners)
    of = np.maximum(np.maximum(labels[:-1, :-1], labels[:-1, 1:]), np.maximum(labels[1:, :-1], labels[1:, 1:]))
    np.add.at(area2, of[cnt == 4], 2)
    np.add.at(area2, of[cnt == 3], 1)
    return area2


def component_filter(C2, min_area):
    """step 6 -> (G, clean, the sorted doubled areas of G's components)"""
    G = outer_filled(C2)
    labels, n = components(G)
    area2 = doubled_areas(G, labels, n)
    keep = area2 >= 2 * max(1, int(min_area))
    keep[0] = False
    return G, keep[labels], sorted(area2[1:].tolist())


def merge(P, C0, near, sclose, opening, min_area):
    """steps 4-7 with the three elements given as (rows, kw, kh) -> dict of C1, C2, G, clean, M"""
    C1 = C0 & dilate_rows(P, *near) & ~P
    closed = erode_rows(dilate_rows(C1, *sclose), *sclose)
    C2 = dilate_rows(erode_rows(closed, *opening), *opening)
    G, clean, areas = component_filter(C2, min_area)
    return {"C1": C1, "C2": C2, "G": G, "clean": clean, "M": P | clean, "areas": areas}


def shadow(img, raw, params, sp, shape=None):
    """the whole of MSK-SHADOW v1 for one image -> dict of P, C0, C1, C2, G, clean, M (boolean planes) and count"""
    P = np.zeros(shape, bool) if raw is None else mk.close(np.asarray(raw) > params.thresh, params.close)
    w = maskfinish.gaussian_weights(sp.sigma)
    C0 = candidates(img, w[len(w) // 2:], sp.t, sp.delta_min, sp.sat_max)
    k, close_k = maskfinish.shadow_sizes(int(P.sum()), sp.near_px)
    out = merge(P, C0, ellipse(k), ellipse(close_k), ellipse(3), sp.min_area)
    out.update(P=P, C0=C0, count=int(out["M"].sum()))
    return out


def finish_with_shadow(img, raw, params, sp, add=None, kind="mask", invert=True, shape=None):
    """M into MSK-SPEC steps 2-6 (the close is done): maskfinish_np.finish on M"""
    import dataclasses
    M = shadow(img, raw, params, sp, shape)["M"]
    rest = dataclasses.replace(params, close=1, thresh=0)
    return mk.finish(np.where(M, 255, 0).astype(np.uint8), rest, add, img, kind, invert, M.shape)


def elements_of(job, count):
    """the three elements of a maskshadow_cases.Job as (rows, kw, kh): its own, or the ellipses the person count gives"""
    k, close_k = maskfinish.shadow_sizes(count, job.near_px)
    return job.near or ellipse(k), job.sclose or ellipse(close_k), job.opening or ellipse(3)


def run_job(job):
    """a maskshadow_cases.Job through every step -> dict of P, C0, C1, C2, G, clean, M, count_p, count"""
    P = mk.close(np.asarray(job.raw) > job.thresh, job.close)
    C0 = candidates(job.img, job.half, job.t, job.delta_min, job.sat_max)
    out = merge(P, C0, *elements_of(job, int(P.sum())), job.min_area)
    out.update(P=P, C0=C0, count_p=int(P.sum()), count=int(out["M"].sum()))
    return out
