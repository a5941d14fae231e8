"""VID-FISHEYE v1 restated in NumPy: decoded fisheye planes -> an S x S pinhole view in RGB, step by step as
the spec words it -- geometry, coordinates, weights, sampling.  The last step is tests/vidcolor_np.py's conversion; from the package
nothing is taken.  NumPy has no fma, so every float32 line below is one rounding per operation."""
import functools
import math

import numpy as np

import vidcolor_np as vc

F32 = np.float32
SENSOR_MM = 36.0
T8 = F32(float.fromhex("0x1.a8279ap-2"))
C1, C2, C3, C4, C5 = (F32(v) for v in (-0.33333316445350647, 0.199985072016716, -0.14244139194488525, 0.10597943514585495,
                                       -0.06087981536984444))
PI4 = F32(math.pi / 4)
LIMIT = F32(2.0 ** 24)


def geometry(focal_mm, size, input_fov):
    """18.1 -> (ifov, hfov, vfov) in degrees, clamped, six decimals"""
    six = lambda v: float("{:.6f}".format(v))
    hfov = min(max(math.degrees(2.0 * math.atan(SENSOR_MM / (2.0 * focal_mm))), 1.0), 179.0)
    vfov = math.degrees(2.0 * math.atan(math.tan(math.radians(hfov) / 2.0) * (size / float(size))))
    vfov = min(max(vfov, 1.0), 179.0)
    return six(min(max(float(input_fov), 1.0), 360.0)), six(hfov), six(vfov)


def constants(projection, S, W, H, ifov, hfov, vfov):
    """18.2: the float32 constants, each a float64 expression rounded once"""
    rad = math.pi / 180.0
    if projection == "equisolid":
        s = math.sin(ifov * rad / 4.0)
        kx, ky = (W / 2.0) / s, (H / 2.0) / s
    else:
        kx, ky = W / (ifov * rad), H / (ifov * rad)
    return dict(tx=F32(math.tan(hfov * rad / 2.0) / S), ty=F32(math.tan(vfov * rad / 2.0) / S),
                kx32=F32(32.0 * kx), ky32=F32(32.0 * ky), kx16=F32(16.0 * kx), ky16=F32(16.0 * ky),
                ox32=F32(16 * W - 16), oy32=F32(16 * H - 16), ox16=F32(8 * W - 16), oy16=F32(8 * H - 16))


def atan_pos(h):
    """EQ-SPEC's reduction and polynomial for atan2(h, 1), h >= 0, without fma"""
    one = np.ones_like(h)
    steep = h > one
    mx, mn = np.where(steep, h, one), np.where(steep, one, h)
    big = mn > T8 * mx
    num = np.where(big, mn - mx, mn)
    den = np.where(big, mn + mx, mx)
    t = num / den
    z = t * t
    p = C5 * z + C4
    p = p * z + C3
    p = p * z + C2
    p = p * z + C1
    r0 = (p * z) * t + t
    k = big.astype(np.int32)
    r0 = np.where(steep, -r0, r0)
    k = np.where(steep, 2 - k, k)
    out = k.astype(F32) * PI4 + r0
    assert out.dtype == F32
    return out


def quant(a, k, o):
    v = a * k + o
    assert v.dtype == F32
    return np.rint(np.minimum(np.maximum(v, -LIMIT), LIMIT)).astype(np.int64)


def coordinates(projection, S, W, H, ifov, hfov, vfov):
    """18.2 -> dict of S x S int64 arrays sx, sy (luma), cx, cy (an axis subsampled by two) and the bool array visible"""
    c = constants(projection, S, W, H, ifov, hfov, vfov)
    n = (2 * np.arange(S) + 1 - S).astype(F32)
    x, y = (n * c["tx"])[None, :], (n * c["ty"])[:, None]
    q = x * x + y * y
    if projection == "equisolid":
        r = np.sqrt(F32(1.0) + q)
        d = (F32(2.0) * r) * (r + F32(1.0))
        g = F32(1.0) / np.sqrt(d)
    else:
        h = np.sqrt(q)
        th = atan_pos(h)
        g = np.where(h > 0, th / np.where(h > 0, h, F32(1.0)), F32(1.0)).astype(F32)
    assert g.dtype == F32
    xg, yg = x * g, y * g
    out = dict(sx=quant(xg, c["kx32"], c["ox32"]), sy=quant(yg, c["ky32"], c["oy32"]),
               cx=quant(xg, c["kx16"], c["ox16"]), cy=quant(yg, c["ky16"], c["oy16"]))
    out["visible"] = (out["sx"] >= -16) & (out["sx"] < 32 * W - 16) & (out["sy"] >= -16) & (out["sy"] < 32 * H - 16)
    return out


@functools.lru_cache(maxsize=None)
def weights():
    """18.3: int64 [32][4], integer arithmetic only"""
    tab = np.zeros((32, 4), np.int64)
    for f in range(32):
        N = (-2048 * f + 96 * f ** 2 - f ** 3, 196608 - 3072 * f - 192 * f ** 2 + 3 * f ** 3, 6144 * f + 96 * f ** 2 - 3 * f ** 3,
             -1024 * f + f ** 3)
        for k, n in enumerate(N):
            q, r = divmod(n, 12)
            tab[f, k] = q + (1 if r > 6 or (r == 6 and q % 2) else 0)
        tab[f, 1 if f <= 16 else 2] += 16384 - tab[f].sum()
    return tab


def sample_plane(plane, cx, cy, vmax):
    """18.3: one plane at the 1/32-px coordinates (cx, cy), int64 arrays of any shape -> int64 samples"""
    P = np.minimum(np.asarray(plane).astype(np.int64), vmax)
    ph, pw = P.shape
    w = weights()
    ix, iy, wx, wy = cx >> 5, cy >> 5, w[cx & 31], w[cy & 31]
    v = np.zeros(cx.shape, np.int64)
    for m in range(4):
        row = np.clip(iy - 1 + m, 0, ph - 1)
        r = np.zeros(cx.shape, np.int64)
        for k in range(4):
            r += wx[..., k] * P[row, np.clip(ix - 1 + k, 0, pw - 1)]
        assert np.abs(r).max(initial=0) < 2 ** 31
        v += wy[..., m] * r
    return np.clip((v + (1 << 27)) >> 28, 0, vmax)


def render(y, u, v, depth, sub, projection, S, ifov, hfov, vfov, full_range=False, keep_rec709=False, rows=None):
    """planes -> S x S x 3 (uint8 or uint16); invisible pixels are black.  rows: a slice, to render those rows of the view only"""
    H, W = y.shape
    sx, sy = vc.SUBS[sub]
    assert u.shape == v.shape == vc.chroma_shape(H, W, sub)
    c = coordinates(projection, S, W, H, ifov, hfov, vfov)
    if rows is not None:
        c = {k: a[rows] for k, a in c.items()}
    vmax = (1 << depth) - 1
    ux, uy = (c["cx"] if sx else c["sx"]), (c["cy"] if sy else c["sy"])
    vis = c["visible"]
    # invisible pixels are not sampled by the kernel; here they are, at a harmless coordinate, and blacked out afterwards
    pick = lambda a: np.where(vis, a, 0)
    Y = sample_plane(y, pick(c["sx"]), pick(c["sy"]), vmax)
    U = sample_plane(u, pick(ux), pick(uy), vmax)
    V = sample_plane(v, pick(ux), pick(uy), vmax)
    out = vc.convert_triples(Y, U, V, depth, full_range, keep_rec709)
    out[~vis] = 0
    return out
