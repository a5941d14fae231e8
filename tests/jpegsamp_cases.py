"""The files the 4:2:2 / 4:4:0 / 4:1:1 decoder tests share.  Per mode 78 files from tests/jpegsamp_np.py's writer (13 sizes that
straddle the 16 x 8 / 8 x 16 / 32 x 8 MCU edges and the 64 x 128 reconstruction tile's seams in both directions, noise and smooth,
quality 100 / 90 / 30, restart intervals of 0, 1, 3 and 7 MCUs in turn), and for 4:2:2 the 234 files Pillow writes for the same
sizes, contents and qualities: plain, optimised tables, restart_marker_blocks=3."""
import itertools

import jpegdec_cases as cases
import jpegsamp_np as samp

SIZES = [(1, 1), (2, 2), (8, 8), (9, 15), (15, 9), (16, 17), (17, 16), (37, 53), (33, 130), (130, 33), (64, 129), (65, 255), (66, 257)]
RESTARTS = (0, 1, 3, 7)
MODES = tuple(samp.SAMPLINGS)            # "4:2:2", "4:4:0", "4:1:1"

_WRITTEN, _PILLOW = {}, []


def written(mode):
    """-> [(name, file bytes)] of one mode, by the NumPy writer"""
    if mode not in _WRITTEN:
        hs, vs = samp.SAMPLINGS[mode]
        out = []
        for k, ((h, w), kind, q) in enumerate(itertools.product(SIZES, ("noise", "smooth"), (100, 90, 30))):
            ri = RESTARTS[k % 4]
            out.append((f"{mode}-{h}x{w}-{kind}-q{q}-ri{ri}", samp.write(cases.image(h, w, kind), hs, vs, q, ri)))
        _WRITTEN[mode] = out
    return _WRITTEN[mode]


def pillow_422():
    """-> [(name, file bytes)]: Pillow's subsampling=1"""
    if not _PILLOW:
        for (h, w), kind, q, mode in itertools.product(SIZES, ("noise", "smooth"), (100, 90, 30), cases.MODES):
            _PILLOW.append((f"pil422-{h}x{w}-{kind}-q{q}-{mode}", cases.encode(cases.image(h, w, kind), quality=q, subsampling=1, **cases.MODES[mode])))
    return _PILLOW


def matrix():
    """every file of the matrix: 3 x 78 written + 234 by Pillow"""
    return [f for mode in MODES for f in written(mode)] + pillow_422()
