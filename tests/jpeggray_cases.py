"""What the gray-mode JPEG decoder tests share: the expected plane and one file per chroma layout."""
import numpy as np

import jpegdec_cases as cases
import jpegsamp_np as samp

LAYOUTS = ("gray", "4:4:4", "4:2:0") + tuple(samp.SAMPLINGS)      # + "4:2:2", "4:4:0", "4:1:1"


def expected_gray(data):
    """FS-SPEC's gray of Pillow's pixels for the file: (4899 R + 9617 G + 1868 B + 8192) >> 14 on int32, Pillow's L array for a gray file"""
    a = cases.pillow(data)
    if a.ndim == 2:
        return a
    a = a.astype(np.int32)
    return ((a[:, :, 0] * 4899 + a[:, :, 1] * 9617 + a[:, :, 2] * 1868 + 8192) >> 14).astype(np.uint8)


def write(img, layout, quality=90, restart=0):
    """img: H x W x 3 uint8 -> the bytes of a baseline JPEG file of the layout (Pillow writes gray, 4:4:4 and 4:2:0, the NumPy writer
    the others)"""
    if layout == "gray":
        return cases.encode(img[:, :, 1].copy(), quality=quality)
    if layout in ("4:4:4", "4:2:0"):
        kw = {"restart_marker_blocks": restart} if restart else {}
        return cases.encode(img, quality=quality, subsampling=0 if layout == "4:4:4" else 2, **kw)
    hs, vs = samp.SAMPLINGS[layout]
    return samp.write(img, hs, vs, quality, restart)
