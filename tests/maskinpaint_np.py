"""MSK-INPAINT v1 restated in NumPy, from the spec's text and not from the kernels: Telea's weights with a
level-ordered march.  `inpaint` computes a level's pixels at once (arrays of float32, one rounding per operation); `inpaint_loop` is
the same text pixel by pixel and offset by offset, and the CPU tests hold the two equal.  Both assert the spec's invariant: every
pixel of F has an offset whose pixel lies at a lower level."""
import math

import numpy as np

MAX_LEVEL = 4095
f32 = np.float32


def offsets(radius):
    """-> [(dy, dx, |r|, 1 / |r|^2)]: the offsets with 0 < dy^2 + dx^2 <= radius^2 in row-major order, the two numbers in double
    rounded to float32"""
    out = []
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            d = dy * dy + dx * dx
            if 0 < d <= radius * radius:
                out.append((dy, dx, f32(math.sqrt(float(d))), f32(1.0 / float(d))))
    return out


def distance2(F):
    """F: H x W bool -> the exact squared distance (int64) of every pixel of F to the nearest pixel outside F, 0 outside F; None when
    the image has no pixel outside F.  Integers only: the vertical distance per column, then the lower envelope along each row."""
    F = np.asarray(F, bool)
    H, W = F.shape
    if F.all():
        return None
    far = np.int64(4 * (H + W + 1))                      # its square is above any real distance and does not overflow
    vert = np.full((H, W), far, np.int64)
    run = np.full(W, far, np.int64)
    for y in range(H):
        run = np.where(F[y], np.minimum(run + 1, far), 0)
        vert[y] = run
    run = np.full(W, far, np.int64)
    for y in range(H - 1, -1, -1):
        run = np.where(F[y], np.minimum(run + 1, far), 0)
        vert[y] = np.minimum(vert[y], run)
    xs = np.arange(W, dtype=np.int64)
    dx2 = (xs[:, None] - xs[None, :]) ** 2               # [x, x']
    d2 = np.empty((H, W), np.int64)
    for y in range(H):
        d2[y] = (dx2 + (vert[y] ** 2)[None, :]).min(axis=1)
    return np.where(F, d2, 0)


def levels(d2):
    """-> L: the smallest k with k^2 >= d2, in integers"""
    d2 = np.asarray(d2, np.int64)
    k = np.floor(np.sqrt(d2.astype(np.float64))).astype(np.int64)
    k = np.where(k * k < d2, k + 1, k)
    k = np.where(k * k < d2, k + 1, k)
    k = np.where((k > 0) & ((k - 1) * (k - 1) >= d2), k - 1, k)
    assert ((k * k >= d2) & ((k == 0) | ((k - 1) * (k - 1) < d2))).all()
    return k


def prepare(F):
    """-> (L, T, K) or None for an F that is empty or covers the image; raises ValueError for K > MAX_LEVEL"""
    F = np.asarray(F) > 0
    if not F.any():
        return None
    d2 = distance2(F)
    if d2 is None:
        return None
    L = levels(d2)
    K = int(L.max())
    if K > MAX_LEVEL:
        raise ValueError(f"K = {K} above {MAX_LEVEL}")
    return L, np.sqrt(d2.astype(f32)), K


def _grad_T(T):
    """central differences of T with clamped indices, times 0.5 -> (gx, gy)"""
    H, W = T.shape
    xs, ys = np.arange(W), np.arange(H)
    gx = f32(0.5) * (T[:, np.minimum(xs + 1, W - 1)] - T[:, np.maximum(xs - 1, 0)])
    gy = f32(0.5) * (T[np.minimum(ys + 1, H - 1), :] - T[np.maximum(ys - 1, 0), :])
    return gx, gy


def inpaint(img, F, radius=5, use_gradient=True):
    """img: H x W x 3 uint8, F: H x W (set where > 0) -> (the filled image, K).  use_gradient = False drops the image-gradient term
    (the tests show that the ramps need it)."""
    img = np.array(img, np.uint8)
    pre = prepare(F)
    if pre is None:
        return img, 0
    L, T, K = pre
    H, W = L.shape
    gxT, gyT = _grad_T(T)
    offs = offsets(radius)
    # a margin around the planes stands for "outside the image": its level is above every k, so it is never read as known
    m = radius + 1
    Lp = np.full((H + 2 * m, W + 2 * m), MAX_LEVEL + 2, np.int64)
    Lp[m:-m, m:-m] = L
    Tq = np.zeros((H + 2 * m, W + 2 * m), f32)
    Tq[m:-m, m:-m] = T
    vals = np.zeros((H + 2 * m, W + 2 * m, 3), f32)
    vals[m:-m, m:-m] = img
    order = np.argsort(L, axis=None, kind="stable")
    starts = np.searchsorted(L.reshape(-1)[order], np.arange(K + 2))
    for k in range(1, K + 1):
        ys, xs = np.unravel_index(order[starts[k]:starts[k + 1]], (H, W))
        if not len(ys):
            continue
        Tp, gx, gy = T[ys, xs], gxT[ys, xs], gyT[ys, xs]
        acc = np.zeros((len(ys), 3), f32)
        s = np.zeros(len(ys), f32)
        for dy, dx, rlen, inv2 in offs:
            qy, qx = ys + (dy + m), xs + (dx + m)        # in the planes with the margin
            use = Lp[qy, qx] < k                         # inside the image at a lower level: its value is final
            if not use.any():
                continue
            rx, ry = f32(-dx), f32(-dy)
            dirv = np.abs(rx * gx + ry * gy) / rlen
            dirv = np.where(dirv < f32(0.01), f32(1e-6), dirv)
            lev = f32(1.0) / (f32(1.0) + np.abs(Tp - Tq[qy, qx]))
            w = (dirv * inv2) * lev
            v = vals[qy, qx]
            grads = []
            for (by, bx), (ay, ax) in (((qy, qx - 1), (qy, qx + 1)), ((qy - 1, qx), (qy + 1, qx))):
                hb, ha = (Lp[by, bx] < k)[:, None], (Lp[ay, ax] < k)[:, None]
                b, a = vals[by, bx], vals[ay, ax]
                g = np.where(hb & ha, f32(0.5) * (a - b), np.where(ha, a - v, np.where(hb, v - b, f32(0.0))))
                grads.append(g if use_gradient else np.zeros_like(g))
            term = w[:, None] * ((v + grads[0] * rx) + grads[1] * ry)
            acc = np.where(use[:, None], acc + term, acc)
            s = np.where(use, s + w, s)
        assert (s > 0).all(), "a pixel of F without a lower level in reach"
        out = np.clip(np.floor(acc / s[:, None] + f32(0.5)), 0, 255)
        img[ys, xs] = out.astype(np.uint8)
        vals[ys + m, xs + m] = out
    return img, K


def inpaint_loop(img, F, radius=5):
    """the same, one pixel, one offset and one channel at a time"""
    img = np.array(img, np.uint8)
    pre = prepare(F)
    if pre is None:
        return img, 0
    L, T, K = pre
    H, W = L.shape
    offs = offsets(radius)

    def known(y, x, k):
        return 0 <= y < H and 0 <= x < W and L[y, x] < k

    for k in range(1, K + 1):
        for y, x in zip(*np.nonzero(L == k)):
            y, x = int(y), int(x)
            gx = f32(0.5) * (T[y, min(x + 1, W - 1)] - T[y, max(x - 1, 0)])
            gy = f32(0.5) * (T[min(y + 1, H - 1), x] - T[max(y - 1, 0), x])
            acc, s = [f32(0.0)] * 3, f32(0.0)
            for dy, dx, rlen, inv2 in offs:
                qy, qx = y + dy, x + dx
                if not known(qy, qx, k):
                    continue
                rx, ry = f32(-dx), f32(-dy)
                dirv = abs(rx * gx + ry * gy) / rlen
                if dirv < f32(0.01):
                    dirv = f32(1e-6)
                lev = f32(1.0) / (f32(1.0) + abs(T[y, x] - T[qy, qx]))
                w = (dirv * inv2) * lev
                for c in range(3):
                    v = f32(img[qy, qx, c])
                    g = []
                    for (by, bx), (ay, ax) in (((qy, qx - 1), (qy, qx + 1)), ((qy - 1, qx), (qy + 1, qx))):
                        hb, ha = known(by, bx, k), known(ay, ax, k)
                        if hb and ha:
                            g.append(f32(0.5) * (f32(img[ay, ax, c]) - f32(img[by, bx, c])))
                        elif ha:
                            g.append(f32(img[ay, ax, c]) - v)
                        elif hb:
                            g.append(v - f32(img[by, bx, c]))
                        else:
                            g.append(f32(0.0))
                    acc[c] = acc[c] + w * ((v + g[0] * rx) + g[1] * ry)
                s = s + w
            assert s > 0, "a pixel of F without a lower level in reach"
            for c in range(3):
                img[y, x, c] = np.uint8(min(max(np.floor(acc[c] / s + f32(0.5)), 0), 255))
    return img, K


# ---- the fixtures of the CPU, host-check and device tests ----------------------------------------------------------------------
def fixture_mask():
    """the spec's 48 x 40 (W x H) fixture: a disc of radius 9, a 12 x 12 block in the bottom-right corner, a 3-row strip of 7 pixels on the
    top edge: 418 pixels, K = 12"""
    H, W = 40, 48
    yy, xx = np.mgrid[:H, :W]
    F = (yy - 20) ** 2 + (xx - 22) ** 2 <= 81
    F[H - 12:, W - 12:] = True
    F[:3, 10:17] = True
    return F


def ramp(H, W, a, b, c):
    """a x + b y + c on all three channels"""
    yy, xx = np.mgrid[:H, :W]
    return np.stack([a * xx + b * yy + c] * 3, -1).astype(np.uint8)


def photograph(H, W, seed):
    """smooth structure plus a little noise, three different channels"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    ch = [128 + 80 * np.sin(xx / (7.0 + c) + c) * np.cos(yy / (5.0 + 2 * c)) + rng.normal(0, 6, (H, W)) for c in range(3)]
    return np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)


def discs(H, W, centres, r):
    yy, xx = np.mgrid[:H, :W]
    F = np.zeros((H, W), bool)
    for cy, cx in centres:
        F |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    return F
