"""VID-FISHEYE v1 without a GPU: the geometry against hand values, the weight table's properties, the quantised
coordinates of tests/vidfisheye_np.py against the float64 definition (written here, shared with nothing), the mirror symmetry, and
the answers that need no restatement: constant planes and the centre pixel."""
import math

import numpy as np
import pytest

import vidcolor_np as vc
import vidfisheye_np as ref
from gs360 import vidfisheye


def test_geometry_against_hand_values():
    # 2 atan(36 / 16) = 132.075022 degrees; 2 atan(36 / 36) = 90; a 0.01 mm lens is clamped to 179; a 500 degree circle to 360
    assert ref.geometry(8.0, 3840, 190.0) == (190.0, 132.075022, 132.075022)
    assert ref.geometry(18.0, 1000, 180.0) == (180.0, 90.0, 90.0)
    assert ref.geometry(0.01, 64, 180.0)[1:] == (179.0, 179.0)
    assert ref.geometry(8.0, 64, 500.0)[0] == 360.0
    assert ref.geometry(8.0, 64, 0.25)[0] == 1.0
    for focal, size, fov in ((8.0, 3840, 190.0), (18.0, 1000, 180.0), (0.01, 64, 500.0), (123.4, 7, 0.25), (2.345, 333, 187.123456789)):
        for proj in ("equidistant", "equisolid"):
            v = vidfisheye.view_from_args(focal, size, proj, fov)
            assert (v.input_fov_deg, v.h_fov_deg, v.v_fov_deg) == ref.geometry(focal, size, fov) and (v.projection, v.size) == (proj, size)
    with pytest.raises(ValueError):
        vidfisheye.view_from_args(8.0, 64, "fisheye", 180.0)


def test_mode_from_env():
    assert vidfisheye.mode_from_env({}) is False and vidfisheye.mode_from_env({"GS360_V2F_FISHEYE": ""}) is False
    assert vidfisheye.mode_from_env({"GS360_V2F_FISHEYE": "device"}) is True
    for bad in ("host", "1", "Device", "device "):
        with pytest.raises(ValueError):
            vidfisheye.mode_from_env({"GS360_V2F_FISHEYE": bad})


def lagrange(t):
    """v360's cubic: the Lagrange basis on the nodes -1, 0, 1, 2"""
    return np.array([-t * (t - 1) * (t - 2) / 6.0, (t + 1) * (t - 1) * (t - 2) / 2.0, -(t + 1) * t * (t - 2) / 2.0, (t + 1) * t * (t - 1) / 6.0])


def test_weights():
    w = ref.weights()
    assert w.shape == (32, 4) and np.all(w.sum(axis=1) == 16384)
    assert w[0].tolist() == [0, 16384, 0, 0]
    # phase 16: symmetric up to the residue, which goes to w1
    assert w[16, 0] == w[16, 3] and abs(int(w[16, 1]) - int(w[16, 2])) <= 1 and w[16, 1] >= w[16, 2]
    for f in range(32):
        assert np.all(np.abs(w[f] - 16384.0 * lagrange(f / 32.0)) <= 1.0), f
        if f:
            # a mirrored phase has the mirrored weights (the residue of phase 16 is zero)
            assert w[32 - f].tolist() == w[f][::-1].tolist(), f
    assert np.abs(w).max() < 32768                   # int16 in the kernel


def truth(projection, S, W, H, ifov, hfov, vfov):
    """float64: the place of every view pixel in the fisheye image, in pixels with centres at integers"""
    n = (2.0 * np.arange(S) + 1.0 - S) / S
    x, y = (n * math.tan(math.radians(hfov) / 2.0))[None, :], (n * math.tan(math.radians(vfov) / 2.0))[:, None]
    h = np.hypot(x, y)
    theta = np.arctan(h)
    if projection == "equisolid":
        r = np.sin(theta / 2.0) / math.sin(math.radians(ifov) / 4.0)
    else:
        r = theta / (math.radians(ifov) / 2.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        cos, sin = np.where(h > 0, x / h, 0.0), np.where(h > 0, y / h, 0.0)
    return (W / 2.0) * (1.0 + r * cos) - 0.5, (H / 2.0) * (1.0 + r * sin) - 0.5


GEOMETRIES = [(1024, 3840, 3840, 190.0, ref.geometry(8.0, 1024, 190.0)[1], ("equidistant", "equisolid")),
              (1024, 8192, 8192, 180.0, 179.0, ("equidistant", "equisolid")),
              (1024, 2880, 2160, 190.0, ref.geometry(8.0, 1024, 190.0)[1], ("equisolid",)),
              (64, 48, 32, 120.0, 150.0, ("equidistant", "equisolid"))]


@pytest.mark.parametrize("S,W,H,ifov,hfov,projections", GEOMETRIES)
def test_coordinates_against_float64(S, W, H, ifov, hfov, projections):
    """the float32 chain lands within a half step of 1/32 px plus 1/256 px of the float64 definition, on both axes"""
    for projection in projections:
        c = ref.coordinates(projection, S, W, H, ifov, hfov, hfov)
        ux, uy = truth(projection, S, W, H, ifov, hfov, hfov)
        ex, ey = np.abs(c["sx"] / 32.0 - ux).max(), np.abs(c["sy"] / 32.0 - uy).max()
        print(f"{projection} S {S} source {W} x {H}: max |dx| {ex:.5f} |dy| {ey:.5f} px, visible {c['visible'].mean():.3f}")
        assert ex <= 1 / 64 + 1 / 256 and ey <= 1 / 64 + 1 / 256, (projection, ex, ey)
        # the subsampled axis: chroma sample k sits at luma 2k + 1/2
        assert np.abs(c["cx"] / 32.0 - (ux - 0.5) / 2.0).max() <= 1 / 64 + 1 / 256
        assert np.abs(c["cy"] / 32.0 - (uy - 0.5) / 2.0).max() <= 1 / 64 + 1 / 256
        inside = (ux >= -0.5) & (ux < W - 0.5) & (uy >= -0.5) & (uy < H - 0.5)
        assert np.mean(inside != c["visible"]) < 0.01        # they differ only where the truth is next to the border
        if S == 64:
            assert 0.3 < c["visible"].mean() < 0.7             # both branches of the visibility test are taken


def planes(rng, H, W, sub, depth):
    ch, cw = vc.chroma_shape(H, W, sub)
    dt = np.uint8 if depth == 8 else np.uint16
    return tuple(rng.integers(0, 1 << depth, size=s).astype(dt) for s in ((H, W), (ch, cw), (ch, cw)))


@pytest.mark.parametrize("projection", ["equidistant", "equisolid"])
def test_mirror_symmetry(projection):
    """odd W, 4:4:4: the view of the left-right mirrored source is the mirrored view.  16 W - 16 is then a multiple of 32, a mirrored
    phase has the mirrored weights and x g changes its sign exactly, so sx and its mirror image add up to 32 W - 32 wherever the
    float32 sum (x g) k + o is exact on both sides: a small source, as here (at 3841 x 3841, 0.3 % of the pixels are one step of
    1/32 px off their mirror image: two roundings of sums of different size).  The border is half open, so the one
    exception is a pixel at exactly sx = -16: it is visible and its mirror image at 32 W - 16 is not."""
    rng = np.random.default_rng(181)
    S, W, H, view = 40, 33, 21, (120.0, 150.0, 150.0)
    c = ref.coordinates(projection, S, W, H, *view)
    assert np.array_equal(c["sx"] + c["sx"][:, ::-1], np.full((S, S), 32 * W - 32))
    both = c["visible"] & c["visible"][:, ::-1]
    lone = c["visible"] & ~c["visible"][:, ::-1]
    assert both.mean() > 0.3 and np.all(c["sx"][lone] == -16)
    for depth in (8, 10):
        y, u, v = planes(rng, H, W, "444", depth)
        a = ref.render(y, u, v, depth, "444", projection, S, *view)
        b = ref.render(y[:, ::-1], u[:, ::-1], v[:, ::-1], depth, "444", projection, S, *view)
        assert np.array_equal(b[both], a[:, ::-1][both]) and a[both].any()
        assert not b[~c["visible"]].any()


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("sub", ["420", "422", "444"])
def test_constant_planes(depth, sub):
    """every phase's weights sum to 16384, so constant planes come through the interpolation unchanged: every visible pixel is the
    VID-COLOR level of the triple, every other pixel black"""
    s = 1 << (depth - 8)
    for projection in ("equidistant", "equisolid"):
        for Y, U, V in ((100 * s, 90 * s, 160 * s), (235 * s, 128 * s, 128 * s), (16 * s, 240 * s, 16 * s), ((1 << depth) - 1, 0, 77 * s)):
            ch, cw = vc.chroma_shape(32, 48, sub)
            dt = np.uint8 if depth == 8 else np.uint16
            out = ref.render(np.full((32, 48), Y, dt), np.full((ch, cw), U, dt), np.full((ch, cw), V, dt), depth, sub, projection, 64,
                             120.0, 150.0, 150.0)
            vis = ref.coordinates(projection, 64, 48, 32, 120.0, 150.0, 150.0)["visible"]
            want = vc.convert_triples(np.array([Y]), np.array([U]), np.array([V]), depth)[0]
            assert vis.any() and not vis.all()
            assert np.all(out[vis] == want) and np.all(out[~vis] == 0)


@pytest.mark.parametrize("depth", [8, 10])
def test_the_centre_pixel(depth):
    """S, W and H odd, 4:4:4: the centre ray meets the centre sample at phase 0"""
    rng = np.random.default_rng(182 + depth)
    for projection in ("equidistant", "equisolid"):
        for W, H, S in ((33, 5, 7), (1, 1, 1), (47, 31, 63)):
            y, u, v = planes(rng, H, W, "444", depth)
            out = ref.render(y, u, v, depth, "444", projection, S, 180.0, 90.0, 90.0)
            want = vc.convert_triples(y[H // 2, W // 2], u[H // 2, W // 2], v[H // 2, W // 2], depth)
            assert np.array_equal(out[S // 2, S // 2], want)


def test_the_kernels_use_no_scratch():
    """both instantiations: no scratch memory, 72 KiB of tables and 256 bytes of weights in LDS, two workgroups of 8 wavefronts per CU"""
    from test_capi_load import _kernel_resources
    res = _kernel_resources()
    if not res:
        pytest.skip("no kernel_resources.txt next to the library (built without csrc/Makefile)")
    hits = {n: r for n, r in res.items() if "vidfisheye_kernel" in n}
    assert len(hits) == 2, sorted(hits)
    for name, r in hits.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["vgpr"] <= 128 and r["occupancy"] >= 4, (name, r)
        assert r["lds"] == 4 * 16384 + 8 * 1024 + 256, (name, r)
