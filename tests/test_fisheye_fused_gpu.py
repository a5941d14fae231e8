"""The fused dual-fisheye kernel (fe_views_kernel, csrc/gs360_table.hip, through gs360_fisheye_views_u8 / gs360_fisheye_views_border_u8)
against the CPU oracle's restatement of FE-SPEC v1, byte for byte: two lenses in one call, the border colour in valid pixels and with the
mask off, padded / offset / unaligned layouts, more views than one launch, sensors narrower than 8 pixels, the backward ray and other lens
fields of view, the entry point's refusals, and the pair renderer's fused mode against table mode's border convention.

Both sensors are cropped: the sensor edge, not the lens cut-off, bounds validity, so valid pixels have border taps.  Every case that
relies on such a condition asserts it from the oracle's own maps."""
import numpy as np
import pytest

import gs360
from gs360 import dualfisheye
from gs360.fisheye import SensorCalibration
from util import rand_image

pytestmark = pytest.mark.gpu

X = dict(width=96, height=64, f=60.0, cx=1.25, cy=-0.75, k1=0.06, k2=-0.004)                         # no tangential term: V.tang == 0
Y = dict(width=96, height=80, f=44.0, cx=-2.5, cy=1.5, k1=0.08, k2=-0.01, k3=0.002, k4=-0.0003,
         p1=0.0007, p2=-0.0004, b1=1.75, b2=-0.6)                                                   # equal width, different height
SPECS = [(0, 0, 100, 80, 70, 50), (30, -10, 100, 80, 67, 21), (-55, 20, 90, 90, 129, 33), (100, 0, 90, 90, 33, 31)]
BORDERED = [(X, 0), (X, 1), (X, 2), (Y, 1), (Y, 2), (Y, 3)]      # (lens, spec) whose valid pixels have border taps
NARROW = [(dict(width=7, height=9, f=2.2, cx=0.3, cy=-0.2, k1=0.05), (10, 5, 120, 120, 70, 37)),
          (dict(width=6, height=5, f=1.6, k1=0.02, p1=0.001, b1=0.5), (-20, 15, 140, 100, 67, 21))]
BACK = (180, 0, 90, 90, 33, 31)                                  # odd sizes: the centre pixel's ray is exactly backward
TILE_W, TILE_H = 64, 16                                          # kTileW, kTileH of the kernel
GUARD, FILL = 64, 0xA5
_MAPS, _IMAGES = {}, {}


def maps(orc, kw, spec, fov=190.0):
    """-> (mx, my, valid) of the spec oracle, computed once per (lens, view, lens field of view) and never changed"""
    key = (tuple(sorted(kw.items())), tuple(spec), float(fov))
    if key not in _MAPS:
        _MAPS[key] = orc.fisheye_spec_map(orc.make_calib(**kw), *spec, float(fov))
        for a in _MAPS[key]:
            a.setflags(write=False)
    return _MAPS[key]


def image(kw, c, seed):
    key = (kw["height"], kw["width"], c, seed)
    if key not in _IMAGES:
        _IMAGES[key] = rand_image(kw["height"], kw["width"], c=c, seed=seed)
        _IMAGES[key].setflags(write=False)
    return _IMAGES[key]


def border_taps(orc, kw, spec, fov=190.0):
    """valid pixels whose 4 x 4 cubic footprint leaves the sensor"""
    mx, my, valid = maps(orc, kw, spec, fov)
    return int((valid & ((mx < 1) | (mx > kw["width"] - 2) | (my < 1) | (my > kw["height"] - 2))).sum())


def all_border(orc, kw, spec, fov=190.0):
    """pixels none of whose taps lies on the sensor, whatever the interpolator (Lanczos-4 reaches 4 pixels)"""
    mx, my, _valid = maps(orc, kw, spec, fov)
    return (mx < -5) | (mx > kw["width"] + 4) | (my < -5) | (my > kw["height"] + 4)


def expected(orc, kw, img, spec, interp, mask_outside, mask_value, fov=190.0, border=None):
    mx, my, valid = maps(orc, kw, spec, fov)
    out = orc.remap_u8(img, mx, my, interp=interp, border_value=border if border is not None else (mask_value, 0, 0, 0))
    return orc.valid_fill(out, valid, mask_value) if mask_outside else out


def n_tiles(specs):
    return sum(-(-s[4] // TILE_W) * -(-s[5] // TILE_H) for s in specs)


def run_fused(ctx, lenses, views, C, interp, mask_outside=True, mask_value=9, fov=190.0, src_pad=0, src_off=0, dst_pad=0, dst_off=0,
              val_off=0, no_valid=(), border_value=None, slot=0):
    """ONE fisheye_views_dev call.  lenses: [(calibration keywords, H x W x C image)]; views: [(lens index, spec)]; view k's validity
    plane is NULL for k in no_valid.  Source rows are padded by src_pad bytes and start src_off bytes into their buffer; destination
    rows are padded to ONE stride for the call (the widest view's row + dst_pad) and start dst_off bytes in, validity planes (tight by
    the ABI) val_off bytes in; a guard lies behind each.  Everything the call may write is 0xA5 before it.
    -> [(pixels h x w x C, validity h x w or None)] after checking that offsets, row padding and guards are still 0xA5."""
    bufs = []
    try:
        d_src = []
        for kw, img in lenses:
            H, W = kw["height"], kw["width"]
            rows = np.full((H, W * C + src_pad), 0xEE, np.uint8)
            rows[:, :W * C] = img.reshape(H, W * C)
            d_src.append(ctx.to_device(np.concatenate([np.full(src_off, 0xDD, np.uint8), rows.reshape(-1)])))
            bufs.append(d_src[-1])
        stride = max(s[4] for _l, s in views) * C + dst_pad if dst_pad else 0
        dsts, vals = [], []
        for k, (_l, s) in enumerate(views):
            w, h = s[4], s[5]
            dsts.append(ctx.alloc(dst_off + h * (stride or w * C) + GUARD))
            vals.append(None if k in no_valid else ctx.alloc(val_off + h * w + GUARD))
        bufs += dsts + [v for v in vals if v is not None]
        for b in dsts + [v for v in vals if v is not None]:
            ctx.memset(b, FILL, slot)           # asynchronous: on the stream the kernel follows on
        ctx.fisheye_views_dev([d_src[l].ptr + src_off for l, _s in views], [gs360.Calib.make(**lenses[l][0]) for l, _s in views], C,
                              [gs360.View.make(*s) for _l, s in views], fov, [d.ptr + dst_off for d in dsts],
                              valid_outs=[None if v is None else v.ptr + val_off for v in vals], interp=interp,
                              mask_outside=mask_outside, mask_value=mask_value, slot=slot,
                              src_stride=lenses[0][0]["width"] * C + src_pad if src_pad else 0, dst_stride=stride,
                              border_value=border_value)
        out = []
        for k, (_l, s) in enumerate(views):
            w, h = s[4], s[5]
            st = stride or w * C
            raw = ctx.download(dsts[k], (dst_off + h * st + GUARD,), np.uint8, slot)
            rows = raw[dst_off:dst_off + h * st].reshape(h, st)
            assert (raw[:dst_off] == FILL).all() and (raw[dst_off + h * st:] == FILL).all(), f"view {k}: bytes around the image written"
            assert (rows[:, w * C:] == FILL).all(), f"view {k}: row padding written"
            va = None
            if vals[k] is not None:
                vraw = ctx.download(vals[k], (val_off + h * w + GUARD,), np.uint8, slot)
                assert (vraw[:val_off] == FILL).all() and (vraw[val_off + h * w:] == FILL).all(), f"view {k}: bytes around the validity plane written"
                va = vraw[val_off:val_off + h * w].reshape(h, w)
            out.append((np.ascontiguousarray(rows[:, :w * C]).reshape(h, w, C), va))
        return out
    finally:
        for b in bufs:
            ctx.free(b)


def check(orc, got, lenses, views, interp, mask_outside, mask_value, what, fov=190.0, border=None):
    for k, ((l, s), (px, va)) in enumerate(zip(views, got)):
        kw, img = lenses[l]
        want = expected(orc, kw, img, s, interp, mask_outside, mask_value, fov, border)
        if not np.array_equal(px, want):
            bad = np.argwhere(px != want)
            raise AssertionError(f"{what}: view {k} (lens {l}, {s}): {len(bad)} of {px.size} bytes differ, first at {bad[0].tolist()}: "
                                 f"got {px[tuple(bad[0][:2])].tolist()}, want {want[tuple(bad[0][:2])].tolist()}")
        if va is not None:
            assert np.array_equal(va, maps(orc, kw, s, fov)[2].astype(np.uint8)), f"{what}: validity plane of view {k}"


def two_lenses(C):
    return [(X, image(X, C, 101)), (Y, image(Y, C, 202))]


INTERLEAVED = [(l, s) for s in SPECS for l in (0, 1)]           # X, Y, X, Y, ... over the four specs


def test_fixture_views_have_border_taps(orc):
    """the precondition of the border cases below: at least 20 valid pixels with border taps in every (lens, view) they rely on"""
    for kw, i in BORDERED:
        assert border_taps(orc, kw, SPECS[i]) >= 20, (kw["height"], SPECS[i])


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("interp", [0, 1, 2, 4])
def test_two_lenses_interleaved(ctx, orc, interp, C):
    """every view is rendered from ITS lens's image, sensor size and coefficients"""
    for kw, i in BORDERED:
        assert border_taps(orc, kw, SPECS[i]) >= 20
    lenses = two_lenses(C)
    got = run_fused(ctx, lenses, INTERLEAVED, C, interp, mask_outside=True, mask_value=9)
    check(orc, got, lenses, INTERLEAVED, interp, True, 9, f"two lenses interp={interp} C={C}")
    # the test itself: the other lens's image and calibration give another picture
    other = [expected(orc, *lenses[1 - l], s, interp, True, 9) for l, s in INTERLEAVED]
    assert any(not np.array_equal(px, o) for (px, _va), o in zip(got, other))


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("interp", [0, 1, 2, 4])
def test_border_colour_with_the_mask_off(ctx, orc, interp, C):
    """mask_outside = 0: invalid pixels keep what the sampler gave them, the border colour {mask_value, 0, 0, 0} where no tap is inside"""
    lenses = two_lenses(C)
    got = run_fused(ctx, lenses, INTERLEAVED, C, interp, mask_outside=False, mask_value=200)
    check(orc, got, lenses, INTERLEAVED, interp, False, 200, f"mask off interp={interp} C={C}")
    n = 0
    for (l, s), (px, _va) in zip(INTERLEAVED, got):
        far = all_border(orc, lenses[l][0], s)
        n += int(far.sum())
        assert (px[far][:, 0] == 200).all() and (px[far][:, 1:] == 0).all()
    assert n > 0


@pytest.mark.parametrize("aligned", [False, True], ids=["unaligned", "aligned"])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("interp", [1, 2])
def test_padded_offset_layouts(ctx, orc, interp, C, aligned):
    """src_stride = W C + 7; one dst_stride for the call = the widest view's row + 5.  "unaligned": sources 3 bytes, destinations and
    validity planes 1 byte into their buffers -- byte stores (and, for RGB, the byte-reading samplers).  "aligned": dword-aligned bases
    and a dst_stride rounded up to a multiple of 4 -- the vector stores, with the partial last tiles of the 67- and 129-pixel rows next
    to the padding (and, for RGB, the pipelined gathers on rows of odd stride)."""
    views = [(l, s) for l, s in INTERLEAVED if ((X, Y)[l], SPECS.index(s)) in BORDERED]
    assert len(views) == 6 and {s[4] for _l, s in views} >= {67, 129}
    lenses = two_lenses(C)
    widest = max(s[4] for _l, s in views) * C
    pad = 5 + (-(widest + 5) % 4 if aligned else 0)
    assert ((widest + pad) % 4 == 0) == (aligned or C == 3)        # (129 * 3 + 5 is a multiple of 4: there the base offset alone unaligns)
    off = dict(src_off=4, dst_off=0, val_off=0) if aligned else dict(src_off=3, dst_off=1, val_off=1)
    got = run_fused(ctx, lenses, views, C, interp, mask_outside=True, mask_value=9, src_pad=7, dst_pad=pad, **off)
    check(orc, got, lenses, views, interp, True, 9, f"layout aligned={aligned} interp={interp} C={C}")


BATCH_SIZES = [(70, 50), (1, 9), (33, 1), (5, 17), (64, 16), (65, 17), (67, 21), (129, 33), (1, 1), (64, 5), (31, 33), (70, 18),
               (5, 5), (65, 16), (40, 17), (66, 3), (65, 17), (1, 1), (64, 17)]
BATCH = [(1 if k >= 16 else k % 2, SPECS[k % 4][:4] + wh) for k, wh in enumerate(BATCH_SIZES)]


@pytest.mark.parametrize("interp,persist", [(1, -1), (2, -1), (2, 8)])
def test_more_views_than_one_launch(ctx, orc, interp, persist):
    """19 views: the second launch restarts tile_base; NULL validity planes; cubic also with 8 persistent workgroups walking the tiles"""
    assert len(BATCH) == 19 > gs360.capi.MAX_VIEWS
    first, second = [s for _l, s in BATCH[:16]], [s for _l, s in BATCH[16:]]
    assert n_tiles(first) % 8 != 0 and n_tiles(second) % 8 != 0 and n_tiles(first) > 8
    assert BATCH[0][0] == 0 and all(l == 1 for l, _s in BATCH[16:])
    assert {1, 5, 64, 65} <= {s[4] for s in first + second} and {1, 17} <= {s[5] for s in first + second}
    lenses = two_lenses(3)
    with ctx.options(table_persist=persist):
        got = run_fused(ctx, lenses, BATCH, 3, interp, mask_outside=True, mask_value=9, no_valid=(3, 17))
    assert got[3][1] is None and got[17][1] is None and got[16][1] is not None
    check(orc, got, lenses, BATCH, interp, True, 9, f"19 views interp={interp} persist={persist}")


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("interp", [0, 1, 2, 4])
def test_sensors_narrower_than_8(ctx, orc, interp, C):
    """the straight-line samplers in their rolled loop (no pipelined gathers below 8 pixels of width), mask on and off"""
    for kw, spec in NARROW:
        assert border_taps(orc, kw, spec) >= 20 and not maps(orc, kw, spec)[2].all()
        lenses = [(kw, image(kw, C, 303))]
        for mask_outside in (True, False):
            got = run_fused(ctx, lenses, [(0, spec)], C, interp, mask_outside=mask_outside, mask_value=200)
            check(orc, got, lenses, [(0, spec)], interp, mask_outside, 200, f"narrow W={kw['width']} interp={interp} C={C} mask={mask_outside}")


@pytest.mark.parametrize("mask_outside", [True, False])
@pytest.mark.parametrize("interp", [1, 2])
def test_backward_ray_and_lens_fields_of_view(ctx, orc, interp, mask_outside):
    """d == 0: the centre pixel of a view that looks straight back has s = 0 and maps to the principal point; a 360-degree lens
    takes it (and nothing else of that view), a 190-degree lens does not.  Then a view under a 120- and a 220-degree lens."""
    lenses = two_lenses(3)
    views = [(0, BACK), (1, BACK)]
    for kw in (X, Y):
        mx, my, valid = maps(orc, kw, BACK, 360.0)
        assert valid.sum() == 1 and valid[15, 16]
        assert (mx[15, 16], my[15, 16]) == (kw["width"] / 2 + kw["cx"], kw["height"] / 2 + kw["cy"])
        assert not maps(orc, kw, BACK, 190.0)[2].any()
    for fov in (360.0, 190.0):
        got = run_fused(ctx, lenses, views, 3, interp, mask_outside=mask_outside, mask_value=9, fov=fov)
        check(orc, got, lenses, views, interp, mask_outside, 9, f"backward ray lens_fov={fov} interp={interp}", fov=fov)
    views = [(1, SPECS[1])]
    assert 974 <= maps(orc, Y, SPECS[1], 120.0)[2].sum() < maps(orc, Y, SPECS[1], 220.0)[2].sum()
    for fov in (120.0, 220.0):
        got = run_fused(ctx, lenses, views, 3, interp, mask_outside=mask_outside, mask_value=9, fov=fov)
        check(orc, got, lenses, views, interp, mask_outside, 9, f"lens_fov={fov} interp={interp}", fov=fov)


def test_refusals_write_nothing(ctx, orc):
    """each refusal returns its code before anything is launched; the three odd calls that are accepted behave as documented"""
    narrower = dict(X, width=88)
    src = ctx.to_device(image(X, 3, 101))
    dsts = [ctx.alloc(70 * 50 * 3) for _ in range(2)]
    views = [gs360.View.make(*SPECS[0])] * 2
    cx, cn = gs360.Calib.make(**X), gs360.Calib.make(**narrower)
    cases = [("mixed widths, explicit stride", gs360.capi.ERR_ARG, dict(calibs=[cx, cn], src_stride=96 * 3)),
             ("mixed widths", gs360.capi.ERR_UNSUPPORTED, dict(calibs=[cx, cn])),
             ("C = 2", gs360.capi.ERR_ARG, dict(C=2)),
             ("interp = 3", gs360.capi.ERR_UNSUPPORTED, dict(interp=3)),
             ("NULL source", gs360.capi.ERR_ARG, dict(srcs=[src, None])),
             ("NULL destination", gs360.capi.ERR_ARG, dict(dsts=[dsts[0], None]))]
    try:
        for b in dsts:
            ctx.memset(b, FILL)
        for name, code, kw in cases:
            with pytest.raises(gs360.Gs360Error) as exc:
                ctx.fisheye_views_dev(kw.get("srcs", [src, src]), kw.get("calibs", [cx, cx]), kw.get("C", 3), views, 190.0,
                                      kw.get("dsts", dsts), interp=kw.get("interp", 1), src_stride=kw.get("src_stride", 0))
            assert exc.value.code == code, name
            for b in dsts:
                assert (ctx.download(b, (70 * 50 * 3,)) == FILL).all(), name
        ctx.fisheye_views_dev([], [], 3, [], 190.0, [])           # no views: accepted, nothing to do
        for b in dsts:
            assert (ctx.download(b, (70 * 50 * 3,)) == FILL).all()
    finally:
        for b in [src] + dsts:
            ctx.free(b)
    lenses = two_lenses(3)
    for given, taken in ((-5, 0), (300, 255)):                    # mask_value is saturated, for the fill and for the border colour
        got = run_fused(ctx, lenses, INTERLEAVED[:6], 3, 2, mask_outside=True, mask_value=given)
        check(orc, got, lenses, INTERLEAVED[:6], 2, True, taken, f"mask_value={given}")


@pytest.mark.parametrize("mask_outside_model", [True, False])
@pytest.mark.parametrize("C", [3, 1])
def test_pair_renderer_fused_border_follows_table_mode(ctx, orc, C, mask_outside_model):
    """PairRenderer(fused=True) on RGB arrays: cv2's Scalar(mask_value, 0, 0, 0) is BLUE of the reference's BGR image, index 2 here --
    the tuple table mode passes; a one-channel pair keeps it on channel 0"""
    for i in (0, 1, 2):
        assert border_taps(orc, X, SPECS[i]) >= 20
    sensors = {"0": SensorCalibration("0", "equidistant_fisheye", **X)}
    specs = [dict(view_id=f"v{k}", yaw_deg=s[0], pitch_deg=s[1], hfov_deg=s[2], vfov_deg=s[3], width=s[4], height=s[5])
             for k, s in enumerate(SPECS)]
    tables = {f"v{k}": dict(lens_key="XY"[k % 2], yaw_rel_deg=float(s[0])) for k, s in enumerate(SPECS)}
    imgs = {"X": image(X, C, 101), "Y": image(X, C, 404)}
    border = (0, 0, 200, 0) if C == 3 else (200, 0, 0, 0)
    r = dualfisheye.PairRenderer(ctx, sensors, specs, tables, {}, 190.0, fused=True)
    try:
        pair = [imgs[k] if C == 3 else imgs[k][:, :, 0] for k in "XY"]
        out = r.render_pair(pair[0], pair[1], "0", "0", interpolation=2, mask_outside_model=mask_outside_model, mask_value=200)
    finally:
        r.close()
    differs = False
    for k, s in enumerate(SPECS):
        img = imgs["XY"[k % 2]]
        want = expected(orc, X, img, s, 2, mask_outside_model, 200, border=border)
        got = out["perspective"][f"v{k}"]
        assert got.shape == want.shape
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            raise AssertionError(f"view {k}: {len(bad)} bytes differ, first at {bad[0].tolist()}: got {got[tuple(bad[0][:2])].tolist()}, "
                                 f"want {want[tuple(bad[0][:2])].tolist()}")
        differs |= not np.array_equal(want, expected(orc, X, img, s, 2, mask_outside_model, 200, border=(200, 0, 0, 0)))
    assert differs == (C == 3)                                     # the test itself: for RGB the two conventions give different pictures
