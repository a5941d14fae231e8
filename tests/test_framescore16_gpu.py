"""FS-DEPTH16 v1 on the MI355X: gs360_frame_stats_u16 against the int64 model (tests/framescore16_np.py), every field exactly and the
fft input's planes bit for bit; gs360_frame_edge_u16 and gs360_frame_flow_u16 against their _u8 twins on the frames' 8-bit view."""
import numpy as np
import pytest

import frame_layouts as layouts
import framescore16_np as fnp16
import framescore_np as fnp
from gs360 import capi, frameflow, framescore

pytestmark = pytest.mark.gpu


def _frame(rng, H, W, C, kind="random"):
    shape = (H, W) if C == 1 else (H, W, C)
    if kind == "random":
        return rng.integers(0, 65536, size=shape, dtype=np.uint16)
    yy, xx = np.mgrid[:H, :W]               # structured: ramps, a disc of highlights and noise in the low byte
    g = (xx * 1799 + yy * 771) % 65536
    g = np.where((xx - W / 3) ** 2 + (yy - H / 2) ** 2 < (min(H, W) / 4) ** 2, 64250, g)
    g = np.clip(g + rng.integers(-700, 701, size=g.shape), 0, 65535).astype(np.uint16)
    return g if C == 1 else np.repeat(g[:, :, None], C, axis=2) ^ (np.arange(C, dtype=np.uint16) * 273)   # the low 10 bits differ


def _bytes(frame):
    """A uint16 frame as the H x W x 2C bytes frame_layouts.upload lays out (host byte order)."""
    H, W = frame.shape[:2]
    return np.ascontiguousarray(frame).view(np.uint8).reshape(H, W, -1)


def _stats(ctx, frames, band, flags, red_index=0, small=None, pad=0):
    """The records (and fft-input planes) of one gs360_frame_stats_u16 call; the records are filled with 0x5A first."""
    H, W = frames[0].shape[:2]
    Cn = layouts.channels(frames[0])
    objs, stride, bufs = layouts.upload(ctx, [_bytes(f) for f in frames], pad)
    stats = ctx.alloc(len(frames) * 104)
    smalls = [ctx.alloc(2 * small[0] * small[1] * 4) for _ in frames] if small else None
    try:
        ctx.memset(stats, 0x5A)
        ctx.frame_stats_dev(objs, H, W, Cn, band, stats, flags=flags, smalls=smalls, small_w=small[0] if small else 0,
                            small_h=small[1] if small else 0, red_index=red_index, stride=stride, depth=16)
        ctx.sync(0)
        recs = ctx.download(stats, (len(frames), 13), np.int64)
        planes = [ctx.download(b, (2, small[1], small[0]), np.float32) for b in smalls] if small else None
    finally:
        for b in bufs + [stats] + (smalls or []):
            ctx.free(b)
    return [dict(zip(fnp.FIELDS, map(int, r))) for r in recs], planes


def _assert_planes(img, band, planes, red_index=0):
    area, level = fnp16.fft_input(img, band[0], band[1], red_index)
    assert np.array_equal(planes[0].view(np.uint32), area.view(np.uint32))      # bit for bit
    assert np.array_equal(planes[1], level)


# 67 x 35 and 130 x 3 in both orientations; a cropped band; C, red_index and the two flags in every combination that matters; odd
# row strides (pad bytes behind a row of 2, 6 or 8 bytes per pixel, so that rows start at all four byte offsets of a dword)
CASES = [  # H, W, C, red_index, crop, pad, kind
    (35, 67, 1, 0, 1.0, 0, "random"), (35, 67, 3, 0, 0.8, 0, "random"), (35, 67, 3, 2, 0.6, 0, "structured"),
    (35, 67, 4, 2, 0.8, 0, "random"), (67, 35, 4, 0, 0.8, 0, "structured"), (3, 130, 3, 0, 1.0, 0, "random"),
    (3, 130, 1, 0, 0.8, 0, "structured"), (130, 3, 3, 2, 0.8, 0, "random"), (130, 3, 4, 0, 0.6, 0, "random"),
    (35, 67, 1, 0, 0.8, 1, "random"), (35, 67, 3, 2, 0.8, 3, "structured"), (35, 67, 4, 0, 0.8, 5, "random"),
    (67, 35, 3, 0, 0.8, 7, "random")]


@pytest.mark.parametrize("H,W,C,red,crop,pad,kind", CASES)
@pytest.mark.parametrize("flags", [0, capi.FS_CIRCLE, capi.FS_HIGHLIGHTS, capi.FS_CIRCLE | capi.FS_HIGHLIGHTS])
def test_fields_equal_the_model(ctx, H, W, C, red, crop, pad, kind, flags):
    rng = np.random.default_rng(H * 1000 + W + C)
    img = _frame(rng, H, W, C, kind)
    band = framescore.band_rows(H, crop)
    got, _ = _stats(ctx, [img], band, flags, red, pad=pad)
    want = fnp16.frame_stats(img, *band, bool(flags & capi.FS_CIRCLE), bool(flags & capi.FS_HIGHLIGHTS), red)
    assert got[0] == want
    if kind == "structured" and H * W > 1000:
        assert 0 < want["n_highlight"] < H * W


def test_batch_of_three(ctx):
    rng = np.random.default_rng(3)
    frames = [_frame(rng, 35, 67, 3, "random" if k % 2 else "structured") for k in range(3)]
    band = framescore.band_rows(35, 0.8)
    small = (67, band[1] - band[0])
    got, planes = _stats(ctx, frames, band, capi.FS_HIGHLIGHTS, small=small, pad=3)
    for k, f in enumerate(frames):
        assert got[k] == fnp16.frame_stats(f, *band, False, True), k
        _assert_planes(f, band, planes[k])


@pytest.mark.parametrize("pad", [0, 3])
def test_three_tiles_at_the_staging_limit(ctx, pad):
    """frame_layouts.MAXIMAL (20 x 514 x 4) at 8 bytes per pixel: the middle tile stages 258 pixels, 2064 bytes, which with a row
    start off a dword boundary (the odd stride) makes 517 of the 520 staged dwords, the third load of a row carrying pixel data."""
    H, W, C = layouts.MAXIMAL
    rng = np.random.default_rng(514)
    img = _frame(rng, H, W, C, "random")
    got, _ = _stats(ctx, [img], layouts.MAXIMAL_BAND, capi.FS_CIRCLE | capi.FS_HIGHLIGHTS, red_index=2, pad=pad)
    assert got[0] == fnp16.frame_stats(img, *layouts.MAXIMAL_BAND, True, True, 2)


def test_largest_products(ctx):
    """512 x 512 frames of 0 and 65535.  Columns in turn put every diagonal tap opposite the centre: |lap| = 8 * 65535 at every
    pixel, the largest product there is, and sum_lap2 = 2^18 * (8 * 65535)^2 passes 2^53 (a double would round it).  The
    checkerboard's diagonal neighbours equal the centre, so its Laplacian and Sobel responses are 0 inside and it checks the sums of
    gray and the edges; a coarse checkerboard of 2 x 2 cells has the largest Sobel responses."""
    yy, xx = np.mgrid[:512, :512]
    columns = ((xx & 1) * 65535).astype(np.uint16)
    checker = (((xx + yy) & 1) * 65535).astype(np.uint16)
    coarse = ((((xx >> 1) + (yy >> 1)) & 1) * 65535).astype(np.uint16)
    frames = [columns, checker, coarse]
    got, _ = _stats(ctx, frames, (0, 512), capi.FS_HIGHLIGHTS)
    for k, f in enumerate(frames):
        assert got[k] == fnp16.frame_stats(f, 0, 512, False, True), k
    assert got[0]["sum_lap2"] == 512 * 512 * (8 * 65535) ** 2 > 2 ** 53
    assert got[2]["sum_mag2"] > 2 ** 53
    assert got[1]["sum_gray"] == 512 * 256 * 65535


def test_fft_input_planes_bit_for_bit_at_a_fractional_scale(ctx):
    rng = np.random.default_rng(1100)
    H, W = 700, 1100
    img = _frame(rng, H, W, 3, "structured")
    band = framescore.band_rows(H, 0.8)
    small = framescore.fft_input_size(W, band[1] - band[0])
    assert small[0] == 512 and W % small[0] and (band[1] - band[0]) % small[1]
    got, planes = _stats(ctx, [img], band, capi.FS_HIGHLIGHTS, red_index=2, small=small, pad=1)
    assert got[0] == fnp16.frame_stats(img, *band, False, True, 2)
    _assert_planes(img, band, planes[0], 2)
    assert (planes[0][1] >= 243).any() and (planes[0][1] < 243).any()


def test_score_arrays_takes_16_bit_frames(ctx, monkeypatch):
    """The Python seam: uint16 ndarrays and 16-bit DeviceFrames beside 8-bit frames of the same size, fft on the host and on the
    device."""
    monkeypatch.setenv("GS360_FS_DEPTH16", "device")
    rng = np.random.default_rng(77)
    v = rng.integers(0, 256, size=(48, 90), dtype=np.uint8)
    a16 = _frame(rng, 48, 90, 3, "structured")
    buf = ctx.to_device(a16)
    try:
        frames = [v, v.astype(np.uint16) * 257, a16, framescore.DeviceFrame(buf, 48, 90, 3, 0, 16)]
        for fft in ("host", "device"):
            got = framescore.score_arrays(ctx, frames, "hybrid", 0.8, True, True, fft=fft)
            assert got[1] == got[0]                                   # the identity: exact sums, exact float32 products
            assert got[3] == got[2]
            want = fnp16.score(a16, "hybrid", 0.8, True, True)
            for k in range(9):                                        # the fft term: FS-FFT v1's bound on the device
                tol = {"rel": 1e-5, "abs": 1e-3 if fft == "device" else 0.0} if k in (0, 7) else {"rel": 1e-12}
                assert got[2][k] == pytest.approx(want[k], **tol), (fft, k)
        assert np.array_equal(framescore.host_copy(ctx, frames[3]), a16)
    finally:
        ctx.free(buf)


def _edge(ctx, frames, band, depth, red_index=0, pad=0):
    H, W = frames[0].shape[:2]
    Cn = layouts.channels(frames[0])
    objs, stride, bufs = layouts.upload(ctx, [_bytes(f) for f in frames] if depth == 16 else frames, pad)
    out = ctx.alloc(len(frames) * 24)
    try:
        ctx.memset(out, 0x5A)
        ctx.frame_edge_dev(objs, H, W, Cn, band, out, red_index=red_index, stride=stride, depth=depth)
        ctx.sync(0)
        return ctx.download(out, (len(frames), 3), np.int64).tolist()
    finally:
        for b in bufs + [out]:
            ctx.free(b)


@pytest.mark.parametrize("H,W,C,red,crop,pad", [(35, 67, 1, 0, 0.8, 0), (35, 67, 3, 2, 0.8, 3), (67, 35, 4, 0, 0.6, 5),
                                                (20, 514, 4, 2, 0.8, 1), (3, 130, 3, 0, 1.0, 0), (40, 300, 3, 0, 0.8, 7)])
def test_edge_records_equal_those_of_the_8_bit_view(ctx, H, W, C, red, crop, pad):
    rng = np.random.default_rng(H + W * 7 + C)
    frames = [_frame(rng, H, W, C, "random"), _frame(rng, H, W, C, "structured")]
    assert all((f & 255).any() for f in frames)                       # a low byte to drop
    band = framescore.edge_band_rows(H, crop)
    got = _edge(ctx, frames, band, 16, red, pad)
    want = _edge(ctx, [fnp16.view8(f) for f in frames], band, 8, red)
    assert got == want and got[0][2] > 0


def _flow(ctx, frames, depth, crop_ratio, flags, red_index=0, pad=0):
    H, W = frames[0].shape[:2]
    Cn = layouts.channels(frames[0])
    geom = frameflow.flow_geometry(H, W, crop_ratio)
    pairs = [(0, 1), (1, 2), (2, 0)]
    objs, stride, bufs = layouts.upload(ctx, [_bytes(f) for f in frames] if depth == 16 else frames, pad)
    out = ctx.alloc(len(pairs) * frameflow.RECORD_DTYPE.itemsize)
    pts = ctx.alloc(len(pairs) * capi.FLOW_MAX_CORNERS * frameflow.POINT_DTYPE.itemsize)
    try:
        ctx.memset(out, 0x5A)
        ctx.memset(pts, 0)
        ctx.frame_flow_dev(objs, H, W, Cn, geom[:4], geom[4], geom[5], pairs, out, flags=flags, points=pts, red_index=red_index,
                           stride=stride, depth=depth)
        ctx.sync(0)
        return (ctx.download(out, (len(pairs),), frameflow.RECORD_DTYPE),
                ctx.download(pts, (len(pairs), capi.FLOW_MAX_CORNERS), frameflow.POINT_DTYPE))
    finally:
        for b in bufs + [out, pts]:
            ctx.free(b)


def _moving_frames(rng, H, W, C):
    """Three 16-bit frames of one blob texture shifted a pixel or two, with noise in the low byte."""
    yy, xx = np.mgrid[:H + 8, :W + 8]
    tex = np.zeros((H + 8, W + 8))
    for _ in range(60):
        cy, cx, r = rng.uniform(0, H + 8), rng.uniform(0, W + 8), rng.uniform(2, 6)
        tex += rng.uniform(0.3, 1.0) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))
    tex = np.clip(tex / tex.max(), 0, 1)
    out = []
    for dy, dx in ((0, 0), (1, 2), (3, 1)):
        g = (tex[dy:dy + H, dx:dx + W] * 60000).astype(np.uint16) + rng.integers(0, 256, size=(H, W)).astype(np.uint16)
        out.append(g if C == 1 else np.repeat(g[:, :, None], C, axis=2) ^ (np.arange(C, dtype=np.uint16) * 257))
    return out


@pytest.mark.parametrize("H,W,C,red,crop_ratio,flags,pad", [
    (96, 128, 1, 0, 1.0, 0, 0),                 # no resize: the crop itself
    (96, 128, 3, 2, 0.6, capi.FS_CIRCLE, 3),    # cropped, odd stride
    (400, 640, 3, 0, 1.0, 0, 0),                # INTER_AREA by integer factors (2 x 2)
    (300, 500, 4, 0, 0.9, 0, 5)])               # the general area tables
def test_flow_records_and_points_equal_those_of_the_8_bit_view(ctx, H, W, C, red, crop_ratio, flags, pad):
    rng = np.random.default_rng(H * 3 + W + C)
    frames = _moving_frames(rng, H, W, C)
    assert all((f & 255).any() for f in frames)
    got, got_pts = _flow(ctx, frames, 16, crop_ratio, flags, red, pad)
    want, want_pts = _flow(ctx, [fnp16.view8(f) for f in frames], 8, crop_ratio, flags, red)
    assert got.tobytes() == want.tobytes() and got_pts.tobytes() == want_pts.tobytes()
    assert int(got[0]["n_corners"]) > 0 and int(got[0]["n_tracked"]) > 0


def test_flow_arrays_pairs_a_16_bit_frame_with_an_8_bit_one(ctx, monkeypatch):
    monkeypatch.setenv("GS360_FS_DEPTH16", "device")
    rng = np.random.default_rng(9)
    f16 = _moving_frames(rng, 96, 128, 3)
    f8 = [fnp16.view8(f) for f in f16]
    want = frameflow.flow_arrays(ctx, f8, [(0, 1), (1, 2)], 0.8)
    assert frameflow.flow_arrays(ctx, f16, [(0, 1), (1, 2)], 0.8) == want
    assert frameflow.flow_arrays(ctx, [f16[0], f8[1], f16[2]], [(0, 1), (1, 2)], 0.8) == want
    assert want[0] is not None


def test_a_frame_above_the_pixel_bound_is_refused_before_any_launch(ctx):
    """The frames are described, not allocated: the pointer is NULL, so a call that got past its checks would end at the NULL
    check (GS360_ERR_ARG), not in a launch.  No frame of exactly GS360_FS16_MAX_PIXELS + 1 pixels has sides <= 65535; 514 x 65283
    is the smallest one above the bound, 528 x 63552 is the bound itself."""
    assert 528 * 63552 == capi.FS16_MAX_PIXELS < 514 * 65283 == capi.FS16_MAX_PIXELS + 6
    assert not any((capi.FS16_MAX_PIXELS + 1) % d == 0 for d in range((capi.FS16_MAX_PIXELS + 1) // 65535, 65536))
    stats = ctx.alloc(104)
    try:
        for H, W, code in ((514, 65283, capi.ERR_UNSUPPORTED), (65283, 514, capi.ERR_UNSUPPORTED), (528, 63552, capi.ERR_ARG)):
            with pytest.raises(capi.Gs360Error) as exc:
                ctx.frame_stats_dev([layouts.Window(None)], H, W, 1, (0, H), stats, depth=16)
            assert exc.value.code == code, (H, W)
        with pytest.raises(capi.Gs360Error) as exc:              # the 8-bit entry point has no such bound
            ctx.frame_stats_dev([layouts.Window(None)], 514, 65283, 1, (0, 514), stats)
        assert exc.value.code == capi.ERR_ARG
    finally:
        ctx.free(stats)
