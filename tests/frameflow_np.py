"""NumPy restatement of FS-FLOW v1: the FrameSelector's Lucas-Kanade motion value of one frame pair, with
the integer stages exact and the float32 stages op by op in the spec's order, written from the spec (not from the kernel) so
that the GPU tests compare two readings of it.  A helper module of the tests, not a test file."""
import numpy as np

import framescore_np as fnp
from gs360 import frameflow

F32 = np.float32
HALF_WIN = 7                 # (winSize - 1) / 2 with winSize 15
WIN = 15
PAD = 15                     # pyramid / derivative border (winSize)
MAX_CORNERS = 1000
MIN_DIST = 5
K_EIG = 1.0 / 50979600.0     # (1 / (4 * 7 * 255))^2: cornerMinEigenVal's Sobel scale, squared
EPS2 = 0.03 * 0.03           # TERM_CRITERIA_EPS, squared in double as calcOpticalFlowPyrLK does
FLT_EPSILON = F32(1.1920929e-07)


def border(p, n):
    """cv::borderInterpolate, BORDER_REFLECT_101."""
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * n - 2 - p
    return p


def bidx(lo, hi, n):
    return np.array([border(i, n) for i in range(lo, hi)], np.int64)


def _rint_u8(v):
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)       # saturate_cast<uchar>(float): round half to even


def area_general(g, dw, dh):
    """INTER_AREA's general 8U path: float32 row buffers then rows, in the tables' order, saturate_cast at the end."""
    sh, sw = g.shape
    xt = fnp.area_tab(sw, dw)
    kx = max(len(t) for t in xt)
    gf = g.astype(F32)
    buf = np.zeros((sh, dw), F32)
    for k in range(kx):          # buf[dx] += S[si] * alpha; a padded entry adds S[0] * 0 = +0, which changes nothing
        si = np.array([t[k][0] if k < len(t) else 0 for t in xt])
        al = np.array([t[k][1] if k < len(t) else 0 for t in xt], F32)
        buf = buf + gf[:, si] * al
    out = np.zeros((dh, dw), F32)
    for d, yt in enumerate(fnp.area_tab(sh, dh)):
        s = F32(0)
        for si, beta in yt:
            s = s + beta * buf[si]
        out[d] = s
    return _rint_u8(out)


def area_fast(g, kx, ky):
    """INTER_AREA's integer-factor 8U path: exact block sums times float32(1/area), saturate_cast."""
    sh, sw = g.shape
    dh, dw = sh // ky, sw // kx
    s = g[:dh * ky, :dw * kx].astype(np.int64).reshape(dh, ky, dw, kx).sum(axis=(1, 3))
    return _rint_u8(s.astype(F32) * (F32(1) / F32(kx * ky)))


def small_frame(img, geom, circle_on, red_index=0):
    """FS-FLOW step 1-4: (uint8 small gray, bool mask or None).  geom = frameflow.flow_geometry(H, W, crop_ratio)."""
    cx0, cy0, cw, ch, sw, sh = geom
    g = fnp.gray_u8(img, red_index)
    H, W = g.shape
    crop = g[cy0:cy0 + ch, cx0:cx0 + cw]
    if (sw, sh) == (cw, ch):
        small = crop.astype(np.uint8)
    else:
        fast = frameflow.area_fast_factors(cw, ch, sw, sh)
        small = area_fast(crop, *fast) if fast else area_general(crop, sw, sh)
    mask = None
    if circle_on:
        ys = cy0 + fnp.framescore.nearest_index(sh, ch)
        xs = cx0 + fnp.framescore.nearest_index(sw, cw)
        mask = fnp.framescore.circle_mask(H, W, ys, xs)
    return small, mask


# ---- goodFeaturesToTrack ----------------------------------------------------------------------------------------------------
def min_eig(s):
    """cornerMinEigenVal(blockSize 7, ksize 3) on uint8 s: exact Sobel and 7x7 sums, float32 from a, b, c on."""
    h, w = s.shape
    g = s.astype(np.int64)
    ry, rx = bidx(-1, h + 1, h), bidx(-1, w + 1, w)
    p = g[ry][:, rx]
    dx = (p[0:h, 2:] + 2 * p[1:h + 1, 2:] + p[2:, 2:]) - (p[0:h, :w] + 2 * p[1:h + 1, :w] + p[2:, :w])
    dy = (p[2:, 0:w] + 2 * p[2:, 1:w + 1] + p[2:, 2:]) - (p[0:h, 0:w] + 2 * p[0:h, 1:w + 1] + p[0:h, 2:])
    by, bx = bidx(-3, h + 3, h), bidx(-3, w + 3, w)

    def box(v):
        v = v[by][:, bx]
        r = sum(v[k:k + h] for k in range(7))
        return sum(r[:, k:k + w] for k in range(7))
    sxx, sxy, syy = box(dx * dx), box(dx * dy), box(dy * dy)
    a = (sxx.astype(np.float64) * (K_EIG * 0.5)).astype(F32)
    b = (sxy.astype(np.float64) * K_EIG).astype(F32)
    c = (syy.astype(np.float64) * (K_EIG * 0.5)).astype(F32)
    return (a + c) - np.sqrt((a - c) * (a - c) + b * b)


def candidates(eig, mask):
    """-> (keys uint64 sorted as greaterThanPtr: value descending, later address first), plus the threshold."""
    h, w = eig.shape
    sel = mask if mask is not None and mask.any() else None
    maxv = eig[sel].max() if sel is not None else eig.max()
    thr = F32(np.float64(maxv) * 0.01)
    t = np.where(eig > thr, eig, F32(0))
    if h < 3 or w < 3:
        return np.zeros(0, np.uint64)
    d = np.full((h - 2, w - 2), -np.inf, F32)
    for oy in range(3):
        for ox in range(3):
            d = np.maximum(d, t[oy:oy + h - 2, ox:ox + w - 2])
    v = t[1:h - 1, 1:w - 1]
    ok = (v != 0) & (v == d)
    if sel is not None:
        ok &= sel[1:h - 1, 1:w - 1]
    yy, xx = np.nonzero(ok)
    yy, xx = yy + 1, xx + 1
    keys = (v[ok].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (yy * w + xx).astype(np.uint64)
    return np.sort(keys)[::-1]


def select(keys, w, h):
    """The greedy minDistance grid (cell 5, dx^2 + dy^2 < 25 against the 3x3 neighbouring cells), stopping at 1000."""
    gw, gh = (w + MIN_DIST - 1) // MIN_DIST, (h + MIN_DIST - 1) // MIN_DIST
    grid = [[] for _ in range(gw * gh)]
    out = []
    for k in keys:
        idx = int(k & np.uint64(0xFFFFFFFF))
        y, x = divmod(idx, w)
        cx, cy = x // MIN_DIST, y // MIN_DIST
        good = True
        for yy in range(max(0, cy - 1), min(gh - 1, cy + 1) + 1):
            for xx in range(max(0, cx - 1), min(gw - 1, cx + 1) + 1):
                for (px, py) in grid[yy * gw + xx]:
                    if (x - px) ** 2 + (y - py) ** 2 < MIN_DIST * MIN_DIST:
                        good = False
        if good:
            grid[cy * gw + cx].append((x, y))
            out.append((x, y))
            if len(out) == MAX_CORNERS:
                break
    return np.array(out, F32).reshape(-1, 2)


def corners(small, mask):
    """goodFeaturesToTrack(maxCorners 1000, qualityLevel 0.01, minDistance 5, blockSize 7) -> N x 2 float32 (x, y)."""
    h, w = small.shape
    return select(candidates(min_eig(small), mask), w, h)


# ---- pyramids and Lucas-Kanade ------------------------------------------------------------------------------------------------
def pyr_down(g):
    h, w = g.shape
    dh, dw = (h + 1) // 2, (w + 1) // 2
    x = g.astype(np.int64)
    cols = [bidx(2 * 0 + k - 2, 2 * (dw - 1) + k - 1, w)[::2] for k in range(5)]
    wt = (1, 4, 6, 4, 1)
    r = sum(wt[k] * x[:, cols[k]] for k in range(5))
    rows = [bidx(k - 2, 2 * (dh - 1) + k - 1, h)[::2] for k in range(5)]
    s = sum(wt[k] * r[rows[k]] for k in range(5))
    return ((s + 128) >> 8).astype(np.uint8)


def pyramid(small):
    """buildOpticalFlowPyramid(winSize 15, maxLevel 2) -> list of the level images (unpadded); stops when a level would be <= 15."""
    levels = [small]
    h, w = small.shape
    for level in range(3):
        if level:
            levels.append(pyr_down(levels[-1]))
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= WIN or h <= WIN:
            break
    return levels


def padded(g):
    h, w = g.shape
    return g.astype(np.int64)[bidx(-PAD, h + PAD, h)][:, bidx(-PAD, w + PAD, w)]


def scharr(g):
    """calcSharrDeriv: (3,10,3) smoothing and a +-1 difference, int16 (Ix, Iy), then padded with zeros by 15."""
    h, w = g.shape
    x = g.astype(np.int64)
    ry, rx = bidx(-1, h + 1, h), bidx(-1, w + 1, w)
    p = x[ry][:, rx]
    t0 = (p[0:h] + p[2:]) * 3 + p[1:h + 1] * 10      # vertical smoothing, columns -1 .. w
    t1 = p[2:] - p[0:h]
    ix = t0[:, 2:] - t0[:, :w]
    iy = (t1[:, 2:] + t1[:, :w]) * 3 + t1[:, 1:w + 1] * 10
    out = np.zeros((2, h + 2 * PAD, w + 2 * PAD), np.int64)
    out[0, PAD:PAD + h, PAD:PAD + w] = ix.astype(np.int16)
    out[1, PAD:PAD + h, PAD:PAD + w] = iy.astype(np.int16)
    return out


def _descale(v, n):
    return (v + (1 << (n - 1))) >> n


def _weights(a, b):
    one, sc = F32(1), F32(1 << 14)
    w00 = np.rint(((one - a) * (one - b)) * sc).astype(np.int64)
    w01 = np.rint((a * (one - b)) * sc).astype(np.int64)
    w10 = np.rint(((one - a) * b) * sc).astype(np.int64)
    return w00, w01, w10, (1 << 14) - w00 - w01 - w10


def _window(P, ix, iy, w):
    """Bilinear sum of the 15 x 15 window with top-left (ix, iy) of the padded plane P (origin at PAD, PAD), per point."""
    ar = np.arange(WIN)
    yy = (iy[:, None] + PAD + ar[None, :])[:, :, None]
    xx = (ix[:, None] + PAD + ar[None, :])[:, None, :]
    w00, w01, w10, w11 = (v[:, None, None] for v in w)
    return P[yy, xx] * w00 + P[yy, xx + 1] * w01 + P[yy + 1, xx] * w10 + P[yy + 1, xx + 1] * w11


def track(pyr_i, pyr_j, pts):
    """calcOpticalFlowPyrLK(winSize 15, maxLevel 2, criteria (EPS|COUNT, 10, 0.03)) -> (end points N x 2 float32, status bool)."""
    n = len(pts)
    max_level = len(pyr_i) - 1
    status = np.ones(n, bool)
    nxt_pts = np.zeros((n, 2), F32)
    hw = F32(HALF_WIN)
    fs = F32(1.0 / (1 << 20))
    for level in range(max_level, -1, -1):
        I, J = padded(pyr_i[level]), padded(pyr_j[level])
        Dv = scharr(pyr_i[level])
        rows, cols = pyr_i[level].shape
        prev = pts * F32(1.0 / (1 << level))
        nxt = prev.copy() if level == max_level else nxt_pts * F32(2)
        nxt_pts = nxt.copy()
        pp = prev - hw
        ip = np.floor(pp).astype(np.int64)
        act = ~((ip[:, 0] < -WIN) | (ip[:, 0] >= cols) | (ip[:, 1] < -WIN) | (ip[:, 1] >= rows))
        if level == 0:
            status &= act
        ipc = np.where(act[:, None], ip, 0)
        w = _weights(pp[:, 0] - ipc[:, 0].astype(F32), pp[:, 1] - ipc[:, 1].astype(F32))
        ival = _descale(_window(I, ipc[:, 0], ipc[:, 1], w), 9)
        ixv = _descale(_window(Dv[0], ipc[:, 0], ipc[:, 1], w), 14)
        iyv = _descale(_window(Dv[1], ipc[:, 0], ipc[:, 1], w), 14)
        a11 = (ixv * ixv).sum(axis=(1, 2)).astype(np.float64).astype(F32) * fs
        a12 = (ixv * iyv).sum(axis=(1, 2)).astype(np.float64).astype(F32) * fs
        a22 = (iyv * iyv).sum(axis=(1, 2)).astype(np.float64).astype(F32) * fs
        D = a11 * a22 - a12 * a12
        mine = ((a22 + a11) - np.sqrt((a11 - a22) * (a11 - a22) + (F32(4) * a12) * a12)) / F32(2 * WIN * WIN)
        bad = (mine < F32(1e-4)) | (D < FLT_EPSILON)
        if level == 0:
            status &= ~(act & bad)
        act &= ~bad
        with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
            Dinv = F32(1) / D
        nxt = nxt - hw
        pdx = np.zeros(n, F32)
        pdy = np.zeros(n, F32)
        for j in range(10):
            inx = np.floor(nxt).astype(np.int64)
            oob = (inx[:, 0] < -WIN) | (inx[:, 0] >= cols) | (inx[:, 1] < -WIN) | (inx[:, 1] >= rows)
            if level == 0:
                status &= ~(act & oob)
            act &= ~oob
            if not act.any():
                break
            inc = np.where(act[:, None], inx, 0)
            wj = _weights(nxt[:, 0] - inc[:, 0].astype(F32), nxt[:, 1] - inc[:, 1].astype(F32))
            diff = _descale(_window(J, inc[:, 0], inc[:, 1], wj), 9) - ival
            b1 = (diff * ixv).sum(axis=(1, 2)).astype(np.float64).astype(F32) * fs
            b2 = (diff * iyv).sum(axis=(1, 2)).astype(np.float64).astype(F32) * fs
            with np.errstate(over="ignore", invalid="ignore"):
                dx = (a12 * b2 - a22 * b1) * Dinv
                dy = (a12 * b1 - a11 * b2) * Dinv
            m = act
            nxt[m, 0] = nxt[m, 0] + dx[m]
            nxt[m, 1] = nxt[m, 1] + dy[m]
            nxt_pts[m] = nxt[m] + hw
            with np.errstate(over="ignore", invalid="ignore"):
                conv = dx.astype(np.float64) * dx.astype(np.float64) + dy.astype(np.float64) * dy.astype(np.float64) <= EPS2
                half = (j > 0) & (np.abs((dx + pdx).astype(np.float64)) < 0.01) & (np.abs((dy + pdy).astype(np.float64)) < 0.01)
            h = m & ~conv & half
            nxt_pts[h, 0] = nxt_pts[h, 0] - dx[h] * F32(0.5)
            nxt_pts[h, 1] = nxt_pts[h, 1] - dy[h] * F32(0.5)
            act = m & ~conv & ~half
            pdx, pdy = dx, dy
    return nxt_pts, status


def pair_record(p0, p1, status):
    """(n_corners, n_tracked, sum_mag): sqrt(dx^2 + dy^2) in float32 per tracked point, summed in double in point order."""
    d = p1 - p0
    mag = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    s = 0.0
    for v in mag[status]:
        s += float(v)
    return len(p0), int(status.sum()), s


class Frame:
    """One frame's per-frame FS-FLOW state: the small image, its mask, corners and pyramid."""

    def __init__(self, img, geom, circle_on, red_index=0):
        self.small, self.mask = small_frame(img, geom, circle_on, red_index)
        self.corners = corners(self.small, self.mask)
        self.pyr = pyramid(self.small)


def pair(prev, curr):
    """-> (record, corners, end points, status) for Frames prev -> curr."""
    p0 = prev.corners
    if len(p0) == 0:
        return (0, 0, 0.0), p0, p0.copy(), np.zeros(0, bool)
    p1, st = track(prev.pyr, curr.pyr, p0)
    return pair_record(p0, p1, st), p0, p1, st


def flow_values(frames, pairs, crop_ratio, mask_mode, red_index=0):
    """The restatement of frameflow.flow_arrays on uint8 ndarrays of one shape."""
    H, W = np.asarray(frames[0]).shape[:2]
    geom = frameflow.flow_geometry(H, W, crop_ratio)
    cache = {}
    out = []
    for a, b in pairs:
        for k in (a, b):
            if k not in cache:
                cache[k] = Frame(frames[k], geom, mask_mode == "fisheye_circle", red_index)
        rec = pair(cache[a], cache[b])[0]
        out.append(frameflow.value_of(rec))
    return out
