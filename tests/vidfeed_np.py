"""VID-FEED v1's (10, 8) format restated in NumPy: 10-bit Y'CbCr planes -> interleaved uint8 RGB.  The integer
step is VID-COLOR v1's at depth 10 (tests/vidcolor_np.rgb14); the float steps 17.3-17.5 are written out here with the encode table
built for levels 0..255.  From the package it takes the three host-built tables only."""
import functools

import numpy as np

import vidcolor_np as ref
from gs360.vidcolor import encode_table, linear_table, primaries_matrix

F32 = np.float32
OUTMAX = 255


@functools.lru_cache(maxsize=None)
def tables(keep_rec709):
    return primaries_matrix().astype(F32), linear_table(), encode_table(bool(keep_rec709), OUTMAX)


def levels8(q, keep_rec709):
    """17.3-17.5 for an 8-bit destination: 14-bit R'G'B' -> uint8 levels (..., 3), every operation in float32 and in the spec's order"""
    m, lin, enc = tables(bool(keep_rec709))
    r, g, b = (lin[c] for c in q)                               # 17.3: linearise
    out = np.empty(r.shape + (3,), np.uint8)
    for c in range(3):
        l = (m[c, 0] * r + m[c, 1] * g) + m[c, 2] * b           # 17.4: primaries, two roundings of the products' sum in this order
        l = np.minimum(np.maximum(l, F32(0.0)), F32(1.0))
        p = np.sqrt(l) * F32(1024.0)                            # 17.5: the encode cell and the place inside it
        i = np.minimum(p.astype(np.int32), 1023)
        f = p - i.astype(F32)
        e = enc[i, 0] + enc[i, 1] * f
        assert e.dtype == F32
        out[..., c] = np.clip(np.rint(e).astype(np.int64), 0, OUTMAX)
    return out


def convert_triples(Y, U, V, full_range=False, keep_rec709=False):
    return levels8(ref.rgb14(Y, U, V, 10, full_range), keep_rec709)


def convert(y, u, v, sub="420", full_range=False, keep_rec709=False):
    """10-bit planes (H x W and the chroma size of `sub`) -> H x W x 3 uint8; chroma replicated (17.1)"""
    H, W = y.shape
    sx, sy = ref.SUBS[sub]
    assert u.shape == v.shape == ((H + sy) >> sy, (W + sx) >> sx), (u.shape, (H, W), sub)
    yy, xx = np.arange(H)[:, None] >> sy, np.arange(W)[None, :] >> sx
    return convert_triples(y, u[yy, xx], v[yy, xx], full_range, keep_rec709)
