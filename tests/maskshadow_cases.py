"""Seeded fixtures of the shadow-estimate tests (MSK-SHADOW v1): images for the blur and candidate stage at the sizes where the
reflection repeats and the tiles end, planes for the component filter at the shapes where a labelling can go wrong, and a synthetic
photograph for the whole chain."""
from collections import namedtuple

import numpy as np

from gs360 import maskfinish

BlurCase = namedtuple("BlurCase", "img raw sigma t delta_min sat_max")
BLUR_SIZES = [((1, 1), 2), ((1, 37), 2), ((5, 3), 2), ((70, 131), 21), ((200, 333), 21)]   # ((H, W), sigma)
BLUR_LIMIT_SIZES = [((40, 2100), 21), ((150, 70), 63.75), ((9, 2100), 63.75)]
LABEL_SIZES = [(97, 130), (257, 513)]
LABEL_WIDE = (97, 2100)                                  # past two tile columns of every shadow kernel; see wide_label_job
LABEL_WIDE_NAMES = ("spiral", "seams", "rings", "checkerboard")
LABEL_MIN_AREA = 20
LABEL_NAMES = ("spiral", "checkerboard", "rings", "diagonals", "seams", "open-cs", "threshold", "empty", "full")
ON, OFF = (128, 128, 128), (255, 0, 0)                   # S = 0 and S = 255: a pixel's saturation bit carries a plane


def textured(H, W, rng, base=150, spread=40):
    """a low-saturation image: smooth blobs of brightness plus per-pixel noise, the channels a few levels apart"""
    yy, xx = np.mgrid[:H, :W]
    g = base + spread * np.sin(yy / 7.0 + rng.random() * 6) * np.cos(xx / 11.0 + rng.random() * 6) + rng.normal(0, 6, (H, W))
    img = g[:, :, None] + rng.integers(-4, 5, (H, W, 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def blur_cases():
    """-> {name: BlurCase}: per size one image with the default thresholds and dark patches, and the same image with t = 1 and
    delta_min = 0, where the bit is the sign of illum - gray and a differently rounded sum shows"""
    rng = np.random.default_rng(20260301)
    out = {}
    for (H, W), sigma in BLUR_SIZES:
        img = textured(H, W, rng)
        dark = rng.random((H, W)) < 0.3
        img[dark] = (img[dark] * 0.4).astype(np.uint8)
        img[rng.random((H, W)) < 0.05] = (20, 20, 160)    # dark and saturated
        raw = np.zeros((H, W), np.uint8)
        raw[H // 3:H // 3 + max(1, H // 4), W // 3:W // 3 + max(1, W // 4)] = 255
        out[f"{H}x{W}-s{sigma}"] = BlurCase(img, raw, sigma, 0.82, 12, 115)
        out[f"{H}x{W}-s{sigma}-sign"] = BlurCase(textured(H, W, rng, 128, 3), raw, sigma, 1.0, 0, 255)
    return out


def blur_limit_cases():
    """-> {name: BlurCase}, built as blur_cases() builds its own but seeded on their own: a second segment of the row pass (2048
    outputs per workgroup) behind three pixel tile columns, and the largest radius the call takes (sigma 63.75: 511 taps, r = 255) on
    a plane both of whose sides are below it and on a row of a full segment"""
    rng = np.random.default_rng(20261022)
    out = {}
    for (H, W), sigma in BLUR_LIMIT_SIZES:
        img = textured(H, W, rng)
        dark = rng.random((H, W)) < 0.3
        img[dark] = (img[dark] * 0.4).astype(np.uint8)
        img[rng.random((H, W)) < 0.05] = (20, 20, 160)
        raw = np.zeros((H, W), np.uint8)
        raw[H // 3:H // 3 + max(1, H // 4), W // 3:W // 3 + max(1, W // 4)] = 255
        out[f"{H}x{W}-s{sigma}"] = BlurCase(img, raw, sigma, 0.82, 12, 115)
        out[f"{H}x{W}-s{sigma}-sign"] = BlurCase(textured(H, W, rng, 128, 3), raw, sigma, 1.0, 0, 255)
    return out


def spiral(H, W):
    """a one-pixel-wide rectangular spiral with one clear pixel between its turns: one walk that turns right whenever the pixel
    ahead is outside the image or the one behind it is set already"""
    X = np.zeros((H, W), bool)
    y, x, dy, dx = 0, 0, 0, 1
    X[0, 0] = True

    def free(y, x):
        return 0 <= y < H and 0 <= x < W and not X[y, x]
    while True:
        if free(y + dy, x + dx) and (not (0 <= y + 2 * dy < H and 0 <= x + 2 * dx < W) or not X[y + 2 * dy, x + 2 * dx]):
            y, x = y + dy, x + dx
            X[y, x] = True
            continue
        dy, dx = dx, -dy
        if not (free(y + dy, x + dx) and free(y + 2 * dy, x + 2 * dx)):
            return X


def ring(X, y0, x0, y1, x1, t=2):
    X[y0:y1, x0:x1] = True
    X[y0 + t:y1 - t, x0 + t:x1 - t] = False


def label_planes(H, W):
    """-> {name: boolean plane} (min_area LABEL_MIN_AREA)"""
    P = {}
    P["spiral"] = spiral(H, W)
    yy, xx = np.mgrid[:H, :W]
    P["checkerboard"] = (yy + xx) % 2 == 0
    X = np.zeros((H, W), bool)
    for inset in (3, 11, 19):                             # three nested rings and a blob in the innermost hole
        ring(X, inset, inset, H - inset, W - inset)
    X[H // 2 - 3:H // 2 + 3, W // 2 - 3:W // 2 + 3] = True
    P["rings"] = X
    X = np.zeros((H, W), bool)
    n = min(H, W)
    X[np.arange(n), np.arange(n)] = True                  # a pure diagonal: no area
    X[np.arange(n - 1), np.arange(n - 1) + 30] = True     # a staircase: half cells only
    X[np.arange(n - 1), np.arange(n - 1) + 31] = True
    P["diagonals"] = X
    X = np.zeros((H, W), bool)                            # a blob over every crossing of a 16-row and a 32-column seam
    for y in range(16, H - 3, 16):
        for x in range(32, W - 3, 32):
            X[y - 3:y + 3, x - 3:x + 3] = True
    X[47, 61:68] = True                                   # ... two of them joined along a row
    P["seams"] = X
    X = np.zeros((H, W), bool)                            # a "C" that opens onto each border: nothing to fill
    X[0:12, 20] = X[0:12, 40] = True; X[11, 20:41] = True
    X[H - 12:H, 50] = X[H - 12:H, 75] = True; X[H - 12, 50:76] = True
    X[30, 0:12] = X[50, 0:12] = True; X[30:51, 11] = True
    X[60, W - 12:W] = X[85, W - 12:W] = True; X[60:86, W - 12] = True
    ring(X, 40, 60, 58, 90)                               # ... and a closed one beside them, with a diagonal step into a blob
    X[58:62, 90:94] = True
    P["open-cs"] = X
    X = np.zeros((H, W), bool)
    X[10:15, 10:16] = True                                # 5 x 6: 2A = 40 = 2 th
    X[30:35, 10:16] = True
    X[30, 10] = False                                     # a corner cut: 2A = 39
    P["threshold"] = X
    P["empty"] = np.zeros((H, W), bool)
    P["full"] = np.ones((H, W), bool)
    assert tuple(P) == LABEL_NAMES
    return P


def plane_image(X):
    """-> (the image whose saturation bit is X, the raw mask: one pixel outside X, or the corner of a full plane)"""
    img = np.where(X[:, :, None], np.array(ON, np.uint8), np.array(OFF, np.uint8)).astype(np.uint8)
    raw = np.zeros(X.shape, np.uint8)
    clear = np.argwhere(~X)
    y, x = clear[0] if len(clear) else (0, 0)
    raw[y, x] = 255
    return img, raw


def rect_rows(kw, kh):
    return [(0, kw)] * kh, kw, kh


def photograph(H, W, seed, person=True):
    """textured mid-gray ground, a person disc, beside it a soft dark low-saturation patch with a bright spot in it, a dark
    saturated patch and dark specks -> (image, raw mask, the saturated patch as a boolean plane)"""
    rng = np.random.default_rng(seed)
    img = textured(H, W, rng, 150, 12).astype(np.float64)
    yy, xx = np.mgrid[:H, :W]
    cy, cx, r = H // 2, W // 3, max(6, min(H, W) // 7)
    d = np.hypot(yy - cy, xx - cx)
    soft = np.clip(1.5 - np.hypot((yy - cy - r // 2) / (0.7 * r), (xx - cx - 1.5 * r) / (0.9 * r)), 0, 1)     # 1 inside, soft rim
    img *= (1 - 0.6 * np.minimum(1, 2 * soft))[:, :, None]
    spot = (abs(yy - cy - r // 2) <= 6) & (abs(xx - cx - r - 10) <= 6)
    img[spot] = 170
    sat = (abs(yy - cy + r) <= 4) & (abs(xx - cx - int(1.3 * r)) <= 5)
    img[sat] = (15, 15, 130)
    for k in range(6):                                    # specks of 4 x 4 around the person
        a = k * 1.1 + 2.2
        y, x = int(cy + (r + 6) * np.sin(a)), int(cx + (r + 6) * np.cos(a))
        img[y:y + 4, x:x + 4] *= 0.3
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    img[d <= r] = (200, 90, 60)
    raw = ((d <= r) * 255).astype(np.uint8) if person else np.zeros((H, W), np.uint8)
    return img, raw, sat


CHAIN_PARAMS = maskfinish.Params(close=5, expand_pixels=4, edge_fuse_pixels=6, thresh=127)
CHAIN_SHADOW = maskfinish.ShadowParams(near_px=45)

# one image of either shadow call, spelled out: half = the weights from the centre outward; near / sclose / opening = (rows, kw, kh),
# or None for the ellipses the count of P gives (maskfinish.shadow_sizes)
Job = namedtuple("Job", "img raw thresh close half t delta_min sat_max near_px min_area near sclose opening")


def blur_job(c):
    w = maskfinish.gaussian_weights(c.sigma)
    return Job(c.img, c.raw, 127, 5, w[len(w) // 2:], c.t, c.delta_min, c.sat_max, 25, 4, None, None, None)


def ends_job(c):
    """the image of a blur fixture under a filter of the same radius whose only weights are its two outermost taps, 0.5 each (the
    weights are data to the call): after both passes illum is the mean of the four pixels r rows and r columns away, reflected, and
    exact in float32.  With t = 1 and delta_min = 0 the bit compares a pixel with four others, so a staged value taken from one
    place too far left or right, or the far end of a staged row or column read wrong, turns about half the bits it reaches; a
    Gaussian of that radius moves illum by hundredths of a level there, which few bits show"""
    r = len(maskfinish.gaussian_weights(c.sigma)) // 2
    half = np.zeros(r + 1, np.float32)
    half[r] = 0.5
    return Job(c.img, c.raw, 127, 5, half, 1.0, 0.0, 255, 25, 4, None, None, None)


def blur_limit_jobs():
    """-> {name: Job}: blur_limit_cases() as blur_job makes them, and per size the -sign image under ends_job"""
    out = {}
    for name, c in blur_limit_cases().items():
        out[name] = blur_job(c)
        if name.endswith("-sign"):
            j = ends_job(c)
            out[name.split("-")[0] + f"-r{len(j.half) - 1}-ends"] = j
    return out


def label_job(name, X):
    """the plane as C2 of a job: a one-tap filter with t = 2 and delta_min = 0 leaves the saturation bit as C0, a rectangle that
    reaches the whole image from the one person pixel makes the near region everything, 1 x 1 elements leave close and open out
    (the full plane lacks the person's pixel: a 3 x 3 close puts it back)"""
    H, W = X.shape
    img, raw = plane_image(X)
    one = rect_rows(1, 1)
    return Job(img, raw, 127, 1, np.ones(1, np.float32), 2.0, 0.0, 115, 25, LABEL_MIN_AREA, rect_rows(2 * W - 1, 2 * H - 1),
               (maskfinish.structuring_rows(3, 3)[0], 3, 3) if name == "full" else one, one)


def wide_label_job(name, X):
    """label_job for a plane wider than the largest element reaches from one pixel (maskfinish.MAX_EXPAND columns either way): the
    person is one clear pixel of X near the middle of each of as many equal column ranges as it takes, so that the near rectangles
    together still cover every column.  They reach 511 columns, not 512: with a reach of 31 more than a multiple of 32 the window's
    last bit ends a dword and the morph kernel reads the last dword its halo stages (reach / 32 + 2 of them), and a rectangle, whose
    last row is as wide as any, does so in the last row of the staged band, where the host check's sanitizer sees one dword less"""
    H, W = X.shape
    reach = maskfinish.MAX_EXPAND - 1
    assert reach % 32 == 31
    assert 2 * H - 1 <= 2 * reach + 1 and name != "full"
    n = -(-W // (2 * reach + 1))
    clear = np.argwhere(~X)
    raw = np.zeros(X.shape, np.uint8)
    covered = np.zeros(W, bool)
    for k in range(n):
        y, x = clear[np.abs(clear[:, 1] - (2 * k + 1) * W // (2 * n)).argmin()]
        raw[y, x] = 255
        covered[max(0, x - reach):x + reach + 1] = True
    assert covered.all()
    one = rect_rows(1, 1)
    return Job(plane_image(X)[0], raw, 127, 1, np.ones(1, np.float32), 2.0, 0.0, 115, 25, LABEL_MIN_AREA,
               rect_rows(min(2 * W - 1, 2 * reach + 1), 2 * H - 1), one, one)


def photo_job(H, W, seed, person=True):
    img, raw, _sat = photograph(H, W, seed, person)
    w = maskfinish.gaussian_weights(CHAIN_SHADOW.sigma)
    return Job(img, raw, CHAIN_PARAMS.thresh, CHAIN_PARAMS.close, w[len(w) // 2:], CHAIN_SHADOW.t, CHAIN_SHADOW.delta_min,
               CHAIN_SHADOW.sat_max, CHAIN_SHADOW.near_px, CHAIN_SHADOW.min_area, None, None, None)
