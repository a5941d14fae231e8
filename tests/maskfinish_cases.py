"""Seeded fixtures of the mask-finishing tests (MSK-SPEC v1): small masks at the sizes and contents where a bit-plane morphology can
go wrong (dword seams, a last dword with one column, elements wider than the image, strips as tall as the image), one mask past a
single tile in both directions, and the parameter values at which the chain takes another path."""
from collections import namedtuple

import numpy as np

from gs360 import maskfinish

Case = namedtuple("Case", "raw add params")            # raw: H x W uint8 or None with add giving the shape

SIZES = [(1, 1), (1, 70), (70, 1), (5, 31), (17, 32), (40, 33), (9, 63), (33, 64), (26, 65), (37, 97), (12, 13)]   # (H, W)
BIG = (515, 1030)


def content(kind, H, W, rng):
    m = np.zeros((H, W), np.uint8)
    if kind == "corners":                                # the four corners and both sides of every dword seam
        for y in (0, H - 1):
            for x in [0, W - 1] + [x for s in range(32, W, 32) for x in (s - 1, s)]:
                m[y, x] = 255
        m[H // 2, [x for s in range(32, W, 32) for x in (s - 1, s)]] = 200
    elif kind == "disc":
        yy, xx = np.mgrid[:H, :W]
        r = max(1, min(H, W) // 3)
        m[(yy - H // 2) ** 2 + (xx - W // 2) ** 2 <= r * r] = 255
    elif kind == "noise":
        m[rng.random((H, W)) < 0.01] = 255
        m[rng.integers(0, H), rng.integers(0, W)] = 255
    elif kind == "set":
        m[:] = 255
    elif kind == "blobs":                                # a blob 3 px from each edge
        for y, x in ((3, W // 2), (H - 4, W // 3), (H // 2, 3), (H // 3, W - 4)):
            if 0 <= y < H and 0 <= x < W:
                m[max(0, y - 1):y + 2, max(0, x - 1):x + 2] = 255
    return m                                             # "clear": zeros


def add_layer(kind, raw, rng):
    H, W = raw.shape
    a = np.zeros((H, W), np.uint8)
    if kind == "overlap":
        a[raw > 0] = 255
        a[H // 2, :] = 255
    elif kind == "disjoint":
        a[(raw == 0) & (rng.random((H, W)) < 0.05)] = 255
        a[0, W - 1] = 255
    return a


def cases():
    """-> {name: Case}"""
    rng = np.random.default_rng(20260114)
    out = {}
    kinds = ["corners", "disc", "noise", "set", "clear", "blobs"]
    closes, ps, fs = [1, 2, 5, 6], [0, 1, 15, 40], [0, 3, 25, "H"]
    n = 0
    for H, W in SIZES:
        for kind in kinds:
            raw = content(kind, H, W, rng)
            f = fs[(n // 2) % 4]
            f = H if f == "H" else f
            f = f if f <= min(H, W) else min(H, W)       # (1 x 70: the strip is the single row)
            params = maskfinish.Params(close=closes[n % 4], expand_pixels=ps[(n // 3) % 4], edge_fuse_pixels=f, thresh=(0, 127)[n % 2])
            add = [None, "overlap", "disjoint"][n % 3]
            out[f"{H}x{W}-{kind}-c{params.close}-p{params.expand_pixels}-f{f}" + (f"-{add}" if add else "")] = Case(
                raw, add_layer(add, raw, rng) if add else None, params)
            n += 1
    H, W = BIG
    out["big-crowd-p77"] = Case(np.maximum(content("disc", H, W, rng), content("noise", H, W, rng)), None,
                                maskfinish.Params(close=5, expand_mode="percent", expand_percent=7.5, edge_fuse_pixels=25))   # round(77.25)
    out["big-blobs-f25"] = Case(content("blobs", H, W, rng), add_layer("disjoint", np.zeros((H, W), np.uint8), rng),
                                maskfinish.Params(close=6, expand_pixels=15, edge_fuse_pixels=25))
    out["none-add-only"] = Case(None, add_layer("overlap", content("disc", 30, 45, rng), rng), maskfinish.Params())
    out["none-empty"] = Case(None, np.zeros((7, 40), np.uint8), maskfinish.Params(edge_fuse_pixels=7))
    return out


def limit_cases():
    """-> {name: Case}: masks past the kernels' own tiles (1024 pixels of a row per workgroup, 32 dwords per morph tile) at the largest
    element the call takes and with side strips of several dwords.  Seeded on their own: cases() draws nothing from here."""
    rng = np.random.default_rng(20261021)
    out = {}
    raw = np.zeros((140, 1700), np.uint8)                # two seeds: the 1025 x 1025 ellipse's rim lies in both morph tile columns
    raw[70, 30], raw[10, 1650] = 255, 200
    out["140x1700-p512"] = Case(raw, None, maskfinish.Params(close=1, expand_pixels=maskfinish.MAX_EXPAND, edge_fuse_pixels=0))
    raw = content("corners", 33, 2100, rng)              # three pack / count / output tile columns, 65 dword seams
    out["33x2100-corners"] = Case(raw, add_layer("overlap", raw, rng), maskfinish.Params(close=6, expand_pixels=15, edge_fuse_pixels=25, thresh=127))
    raw = np.zeros((210, 1100), np.uint8)                # side strips of seven dwords, spread over 141 rows
    raw[rng.random((210, 1100)) < 0.0005] = 255
    out["210x1100-f200"] = Case(raw, None, maskfinish.Params(close=1, expand_pixels=0, edge_fuse_pixels=200))
    return out


def shape_of(case):
    return (case.raw if case.raw is not None else case.add).shape


def image_for(shape, seed=3):
    return np.random.default_rng(seed).integers(0, 256, shape + (3,), dtype=np.uint8)
