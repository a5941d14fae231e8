"""The files the JPEG decoder tests share: the matrix of DESIGN.md section 12 (228 files written by Pillow) and a few helpers."""
import io
import itertools

import numpy as np

SIZES = [(1, 1), (8, 8), (17, 16), (37, 53), (48, 80), (33, 130)]
MODES = {"plain": {}, "optimize": {"optimize": True}, "restart": {"restart_marker_blocks": 3}}


def image(h, w, kind, gray=False, seed=0):
    if kind == "noise":
        a = np.random.default_rng(1000 * h + w + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    else:
        yy, xx = np.mgrid[:h, :w]
        a = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) * 3 % 256], -1).astype(np.uint8)
    return a[:, :, 1].copy() if gray else a


def encode(a, **kw):
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(a).save(f, "JPEG", **kw)
    return f.getvalue()


def pillow(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


def matrix():
    """-> [(name, file bytes)]: sizes x noise / smooth x 4:4:4 / 4:2:0 x quality 100 / 90 / 30 x plain / optimize / restart, and grayscale"""
    out = []
    for (h, w), kind in itertools.product(SIZES, ("noise", "smooth")):
        for sub, q, mode in itertools.product((0, 2), (100, 90, 30), MODES):
            out.append((f"{h}x{w}-{kind}-s{sub}-q{q}-{mode}", encode(image(h, w, kind), quality=q, subsampling=sub, **MODES[mode])))
        out.append((f"{h}x{w}-{kind}-gray", encode(image(h, w, kind, gray=True), quality=90)))
    return out


_MATRIX = []


def matrix_once():
    if not _MATRIX:
        _MATRIX.extend(matrix())
    return _MATRIX
