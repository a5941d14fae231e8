"""VID-COLOR v1 restated in NumPy: decoded Y'CbCr planes -> interleaved RGB, step by step as the spec words
it.  From the package it takes the three host-built tables only (gs360.vidcolor's builders); the integer coefficients, the chroma
replication and every float32 operation are written out here."""
import functools

import numpy as np

from gs360.vidcolor import encode_table, linear_table, primaries_matrix

F32 = np.float32
KR, KB = 0.2126, 0.0722
SUBS = {"444": (0, 0), "422": (1, 0), "420": (1, 1)}


def coefficients(depth, full_range):
    """17.2: (cy, crv, cgu, cgv, cbu, yoff, coff, vmax), round-to-nearest-even of the real coefficients times 16383 * 2^14"""
    kg = 1.0 - KR - KB
    scale = 16383.0 * 16384.0
    s, vmax = 1 << (depth - 8), (1 << depth) - 1
    dy, dc = (float(vmax), float(vmax)) if full_range else (219.0 * s, 224.0 * s)
    r = lambda v: int(np.rint(v))
    return (r(scale / dy), r((2.0 * (1.0 - KR)) * scale / dc), r((KB * (2.0 * (1.0 - KB)) / kg) * scale / dc),
            r((KR * (2.0 * (1.0 - KR)) / kg) * scale / dc), r((2.0 * (1.0 - KB)) * scale / dc), 0 if full_range else 16 * s, 128 * s, vmax)


@functools.lru_cache(maxsize=None)
def tables(depth, keep_rec709):
    outmax = 255 if depth == 8 else 65535
    return primaries_matrix().astype(F32), linear_table(), encode_table(bool(keep_rec709), outmax), outmax


def rgb14(Y, U, V, depth, full_range):
    """17.2: integer samples (any shape) -> three int64 arrays of 14-bit R'G'B'"""
    cy, crv, cgu, cgv, cbu, yoff, coff, vmax = coefficients(depth, full_range)
    Y, U, V = (np.minimum(np.asarray(a).astype(np.int64), vmax) for a in (Y, U, V))
    yy = cy * (Y - yoff) + 8192
    u, v = U - coff, V - coff
    assert max(int(np.abs(yy).max()) + crv * vmax, int(np.abs(yy).max()) + (cgu + cgv) * vmax, int(np.abs(yy).max()) + cbu * vmax) < 2 ** 31
    return tuple(np.clip(t >> 14, 0, 16383) for t in (yy + crv * v, yy - cgu * u - cgv * v, yy + cbu * u))


def levels(q, depth, keep_rec709):
    """17.3-17.5: 14-bit R'G'B' -> output levels (..., 3), every operation in float32 and in the spec's order"""
    m, lin, enc, outmax = tables(depth, bool(keep_rec709))
    r, g, b = (lin[c] for c in q)
    out = np.empty(r.shape + (3,), np.uint8 if depth == 8 else np.uint16)
    for c in range(3):
        l = (m[c, 0] * r + m[c, 1] * g) + m[c, 2] * b
        l = np.minimum(np.maximum(l, F32(0.0)), F32(1.0))
        p = np.sqrt(l) * F32(1024.0)
        i = np.minimum(p.astype(np.int32), 1023)
        f = p - i.astype(F32)
        e = enc[i, 0] + enc[i, 1] * f
        assert e.dtype == F32
        out[..., c] = np.clip(np.rint(e).astype(np.int64), 0, outmax)
    return out


def convert_triples(Y, U, V, depth, full_range=False, keep_rec709=False):
    return levels(rgb14(Y, U, V, depth, full_range), depth, keep_rec709)


def convert(y, u, v, depth, sub="420", full_range=False, keep_rec709=False):
    """planes (H x W and the chroma size of `sub`) -> H x W x 3; chroma replicated (17.1)"""
    H, W = y.shape
    sx, sy = SUBS[sub]
    assert u.shape == v.shape == ((H + sy) >> sy, (W + sx) >> sx), (u.shape, (H, W), sub)
    yy, xx = np.arange(H)[:, None] >> sy, np.arange(W)[None, :] >> sx
    return convert_triples(y, u[yy, xx], v[yy, xx], depth, full_range, keep_rec709)


def chroma_shape(H, W, sub):
    sx, sy = SUBS[sub]
    return (H + sy) >> sy, (W + sx) >> sx
