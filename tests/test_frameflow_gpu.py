"""gs360_frame_flow_u8 on the MI355X against the FS-FLOW v1 restatement (tests/frameflow_np.py), exactly: every corner in order,
every point's status and float32 end position, and every record; then the drop-in seams of gs360.frameflow on PNG folders."""
import ctypes

import numpy as np
import pytest

import frame_layouts as layouts
import frameflow_np as fnp
from gs360 import capi, framescore, frameflow, imageio

pytestmark = pytest.mark.gpu


def _texture(rng, H, W, C, block=8):
    """A blocky texture with mild noise (corners at block corners), larger than H x W by 16 on each side for shifted crops."""
    hb, wb = (H + 32) // block + 2, (W + 32) // block + 2
    g = np.repeat(np.repeat(rng.integers(0, 256, (hb, wb)), block, 0), block, 1)[:H + 32, :W + 32]
    g = np.clip(g + rng.integers(-4, 5, g.shape), 0, 255).astype(np.uint8)
    if C == 1:
        return g
    return np.stack([g ^ np.uint8(17 * c) for c in range(C)], axis=2)


def _moving(rng, H, W, C, shifts, block=8):
    big = _texture(rng, H, W, C, block)
    return [np.ascontiguousarray(big[16 + dy:16 + dy + H, 16 + dx:16 + dx + W]) for dx, dy in shifts]


def _check(ctx, frames, pairs, crop, mode, red_index=0, dev_frames=None, ref=None):
    """ref: a dict that keeps the restatement's frames and pair results from one call to the next on the same frames and crop."""
    recs, pts = frameflow.flow_records(ctx, dev_frames or frames, pairs, crop, mode, red_index, with_points=True)
    H, W = frames[0].shape[:2]
    geom = frameflow.flow_geometry(H, W, crop)
    cache = {} if ref is None else ref
    for k, (a, b) in enumerate(pairs):
        for f in (a, b):
            if f not in cache:
                cache[f] = fnp.Frame(frames[f], geom, mode == "fisheye_circle", red_index)
        if (a, b) not in cache:
            cache[a, b] = fnp.pair(cache[a], cache[b])
        (nc, nt, s), p0, p1, st = cache[a, b]
        n = int(recs[k]["n_corners"])
        assert n == nc, f"pair {k}: {n} corners, want {nc}"
        got = pts[k][:n]
        np.testing.assert_array_equal(got["x0"], p0[:, 0])
        np.testing.assert_array_equal(got["y0"], p0[:, 1])
        np.testing.assert_array_equal(got["status"].astype(bool), st)
        np.testing.assert_array_equal(got["x1"], p1[:, 0])
        np.testing.assert_array_equal(got["y1"], p1[:, 1])
        assert int(recs[k]["n_tracked"]) == nt
        assert recs[k]["sum_mag"] == s
    return recs


def test_8k_single_frames_general_area_path(ctx):
    rng = np.random.default_rng(1)
    frames = _moving(rng, 4320, 7680, 3, [(0, 0), (5, -3)], block=24)
    geom = frameflow.flow_geometry(4320, 7680, 0.6)
    assert frameflow.area_fast_factors(*geom[2:]) is None
    recs = _check(ctx, frames, [(0, 1)], 0.6, "none")
    v = frameflow.value_of(recs[0])
    assert v is not None and abs(v - np.hypot(5, 3) * geom[4] / geom[2]) < 0.2


def test_3840_pairs_circle_integer_factor_path(ctx):
    rng = np.random.default_rng(2)
    frames = _moving(rng, 3840, 3840, 3, [(0, 0), (12, -12), (-12, 12)], block=24)
    assert frameflow.area_fast_factors(*frameflow.flow_geometry(3840, 3840, 1.0)[2:]) == (12, 12)
    recs = _check(ctx, frames, [(0, 1), (1, 2)], 1.0, "fisheye_circle")
    assert all(r["n_tracked"] > 0 for r in recs)


@pytest.mark.parametrize("H, W, C, red, crop", [(333, 517, 4, 2, 0.6), (401, 263, 3, 2, 1.0), (97, 131, 1, 0, 0.6),
                                                (241, 400, 3, 0, 1.0), (200, 300, 3, 0, 1.0)])
def test_odd_sizes_channels_and_bgr(ctx, H, W, C, red, crop):
    rng = np.random.default_rng(H * W + C)
    frames = _moving(rng, H, W, C, [(0, 0), (2, 1), (-3, 2)], block=6)
    for mode in ("none", "fisheye_circle"):
        _check(ctx, frames, [(0, 1), (1, 2), (2, 0)], crop, mode, red_index=red)


def test_tiny_frames_use_fewer_levels(ctx):
    rng = np.random.default_rng(3)
    for H, W in ((40, 50), (20, 64), (9, 12)):
        frames = _moving(rng, H, W, 1, [(0, 0), (1, 1)], block=3)
        _check(ctx, frames, [(0, 1)], 1.0, "none")


def test_noise_worst_case_and_flat_frame(ctx):
    rng = np.random.default_rng(4)
    noise = rng.integers(0, 256, (320, 320), dtype=np.uint8)
    shifted = np.roll(noise, (1, 2), axis=(0, 1))
    flat = np.full((320, 320), 90, np.uint8)
    recs = _check(ctx, [noise, shifted, flat], [(0, 1), (2, 0), (0, 0)], 1.0, "none")
    assert recs[0]["n_corners"] == 1000
    assert recs[1]["n_corners"] == 0 and frameflow.value_of(recs[1]) is None
    assert recs[2]["sum_mag"] == 0.0 and frameflow.value_of(recs[2]) == 0.0


def test_batch_split_gaps_determinism_and_independence(ctx):
    rng = np.random.default_rng(5)
    frames = _moving(rng, 180, 240, 3, [(k % 5 - 2, k % 3 - 1) for k in range(17)], block=6)
    chain = [(k, k + 1) for k in range(16)]
    gaps = [(0, 2), (5, 3), (16, 0), (4, 4), (9, 16), (1, 15)]
    r1 = _check(ctx, frames, chain + gaps, 1.0, "fisheye_circle")
    r2 = frameflow.flow_records(ctx, frames, chain + gaps, 1.0, "fisheye_circle")
    assert r1.tobytes() == r2.tobytes()
    for k, pr in enumerate(chain + gaps):
        alone = frameflow.flow_records(ctx, frames, [pr], 1.0, "fisheye_circle")
        assert alone.tobytes() == r1[k:k + 1].tobytes()


def test_device_frames(ctx):
    rng = np.random.default_rng(6)
    frames = _moving(rng, 300, 500, 3, [(0, 0), (3, -2)], block=6)
    bufs = [ctx.to_device(f) for f in frames]
    try:
        dev = [framescore.DeviceFrame(b, 300, 500, 3, 0) for b in bufs]
        _check(ctx, frames, [(0, 1)], 0.6, "none", dev_frames=dev)
    finally:
        for b in bufs:
            ctx.free(b)


# ---- row strides and windows ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H, W, C, red, pad, window", [(97, 131, 1, 0, 3, None), (120, 160, 3, 0, 7, None), (120, 160, 4, 2, 2, None),
                                                       (96, 128, 3, 0, 0, (128, 200, 7))])
def test_padded_rows_and_a_window(ctx, H, W, C, red, pad, window):
    rng = np.random.default_rng(H * W + C + pad)
    frames = _moving(rng, H, W, C, [(0, 0), (2, 1), (-3, 2)], block=6)
    if window:
        PH, PW, row = window
        window = (PH, PW, row, layouts.window_column(9, PW * C, row, C))
    objs, stride, bufs = layouts.upload(ctx, frames, pad, window)
    try:
        dev = layouts.device_frames(objs, frames, stride)
        for crop in (0.6, 1.0):
            for mode in ("none", "fisheye_circle"):
                recs = _check(ctx, frames, [(0, 1), (1, 2), (2, 0)], crop, mode, red_index=red, dev_frames=dev)
                assert all(r["n_corners"] > 0 for r in recs), (crop, mode)
    finally:
        for b in bufs:
            ctx.free(b)


def test_device_frames_of_three_strides_in_one_call(ctx):
    """DeviceFrames of one shape stored packed (stride 0 and W*C) and with 8 filler bytes a row: each is read with its own stride,
    also in the pairs that join two strides."""
    rng = np.random.default_rng(61)
    frames = _moving(rng, 61, 90, 3, [(0, 0), (2, 1), (-3, 2)], block=6)
    pairs = [(0, 1), (1, 2), (2, 0)]
    dev, bufs = layouts.mixed_strides(ctx, frames)
    try:
        for mode in ("none", "fisheye_circle"):
            got = _check(ctx, frames, pairs, 1.0, mode, dev_frames=dev)
            assert got.tobytes() == frameflow.flow_records(ctx, frames, pairs, 1.0, mode).tobytes()
            assert all(r["n_tracked"] > 0 for r in got)
    finally:
        for b in bufs:
            ctx.free(b)


# ---- the entry point's scheduler: resident slots, eviction, groups of pairs -------------------------------------------------------
def _windows(rng, H, W, shifts, block=4):
    """Gray H x W frames cut at (dx, dy) = shifts >= 0 from one blocky texture with mild noise, as _moving's, of whatever size the
    shifts need."""
    th, tw = H + max(dy for _, dy in shifts), W + max(dx for dx, _ in shifts)
    g = np.repeat(np.repeat(rng.integers(0, 256, (th // block + 1, tw // block + 1)), block, 0), block, 1)[:th, :tw]
    g = np.clip(g + rng.integers(-4, 5, g.shape), 0, 255).astype(np.uint8)
    return [np.ascontiguousarray(g[dy:dy + H, dx:dx + W]) for dx, dy in shifts]


def test_slot_eviction_and_recomputation(ctx):
    """Forty frames through the 32 resident slots: the chain's second group takes the slots of frames 0..14 (eviction), the third
    names frames 0 and 3 again (recomputation) next to frames that are still resident (17, 20, 30)."""
    frames = _windows(np.random.default_rng(7), 48, 64, [(3 * k, k % 3) for k in range(40)])
    pairs = [(k, k + 1) for k in range(39)] + [(39, 0), (0, 20), (3, 38), (17, 17), (38, 3)]
    recs = _check(ctx, frames, pairs, 1.0, "none")
    assert all(r["n_corners"] > 0 and r["n_tracked"] > 0 for r in recs)          # an all-empty result cannot pass
    assert len({r.tobytes() for r in recs}) == len(pairs)
    for k, pr in enumerate(pairs):
        alone = frameflow.flow_records(ctx, frames, [pr], 1.0, "none")
        assert alone.tobytes() == recs[k:k + 1].tobytes(), pr


def test_more_pairs_than_one_pair_launch(ctx):
    """All 132 ordered pairs of twelve frames: groups of 64, 64 and 4 pairs, the second and third without a new frame."""
    frames = _windows(np.random.default_rng(7), 48, 64, [(3 * k, k % 3) for k in range(12)])
    pairs = [(a, b) for a in range(12) for b in range(12) if a != b]
    ref = {}
    fwd = _check(ctx, frames, pairs, 1.0, "none", ref=ref)
    assert all(r["n_corners"] > 0 and r["n_tracked"] > 0 for r in fwd)
    back = _check(ctx, frames, pairs[::-1], 1.0, "none", ref=ref)
    assert back[::-1].tobytes() == fwd.tobytes()


def test_argument_errors_return_their_codes_without_a_launch(ctx):
    H, W = 40, 330
    buf = ctx.to_device(np.zeros((H, W), np.uint8))
    out = ctx.alloc(2 * 24)
    fn = ctx.L.gs360_frame_flow_u8
    two = (ctypes.c_void_p * 2)(buf.ptr, buf.ptr)
    p01 = (ctypes.c_int * 2)(0, 1)

    def call(frames=two, nf=2, h=H, w=W, c=1, stride=0, red=0, crop=(0, 0, W, H), sw=320, sh=38, flags=0, pairs=p01, n_pairs=1, o=None,
             slot=0):
        return fn(ctx.handle, frames, nf, h, w, c, stride, red, *crop, sw, sh, flags, pairs, n_pairs, out.ptr if o is None else o,
                  None, slot)
    try:
        ctx.memset(out, 0x5A)
        ctx.sync(0)
        ARG, UNSUPPORTED = -1, -4
        assert call(n_pairs=-1) == ARG
        assert call(frames=None) == ARG
        assert call(pairs=None) == ARG
        assert call(o=ctypes.c_void_p(None)) == ARG
        assert call(c=2) == ARG
        assert call(red=1) == ARG
        assert call(h=0) == ARG
        assert call(w=65536) == UNSUPPORTED
        assert call(stride=W - 1) == ARG
        assert call(crop=(-1, 0, W, H)) == ARG
        assert call(crop=(0, -1, W, H)) == ARG
        assert call(crop=(1, 0, W, H)) == ARG
        assert call(crop=(0, 1, W, H)) == ARG
        assert call(crop=(0, 0, 0, H)) == ARG
        assert call(crop=(0, 0, W, 0)) == ARG
        assert call(sw=0) == ARG
        assert call(crop=(0, 0, 100, H), sw=101) == ARG
        assert call(sw=321) == ARG                                     # inside the 330-pixel crop, above GS360_FLOW_MAX_SIDE
        assert call(flags=capi.FS_HIGHLIGHTS) == ARG
        assert call(pairs=(ctypes.c_int * 2)(-1, 0)) == ARG
        assert call(pairs=(ctypes.c_int * 2)(0, 2)) == ARG
        assert call(frames=(ctypes.c_void_p * 2)(buf.ptr, None)) == ARG
        assert call(slot=99) == ARG
        ctx.sync(0)
        assert np.all(ctx.download(out, (48,), np.uint8) == 0x5A)          # nothing ran
        assert call(n_pairs=0) == 0
        ctx.sync(0)
        assert np.all(ctx.download(out, (48,), np.uint8) == 0x5A)
    finally:
        ctx.free(buf)
        ctx.free(out)


def test_a_null_frame_that_no_pair_names_is_accepted(ctx):
    frames = _windows(np.random.default_rng(7), 48, 64, [(0, 0), (3, 1)])
    bufs = [ctx.to_device(f) for f in frames]
    out = ctx.alloc(2 * frameflow.RECORD_DTYPE.itemsize)
    geom = frameflow.flow_geometry(48, 64, 1.0)
    try:
        ctx.memset(out, 0x5A)
        ctx.frame_flow_dev([bufs[0], layouts.Window(None), bufs[1]], 48, 64, 1, geom[:4], geom[4], geom[5], [(0, 2), (2, 0)], out)
        got = ctx.download(out, (2,), frameflow.RECORD_DTYPE)
    finally:
        for b in bufs + [out]:
            ctx.free(b)
    ref = [fnp.Frame(f, geom, False) for f in frames]
    for rec, (a, b) in zip(got, [(0, 1), (1, 0)]):
        nc, nt, s = fnp.pair(ref[a], ref[b])[0]
        assert (int(rec["n_corners"]), int(rec["n_tracked"]), rec["sum_mag"]) == (nc, nt, s) and nc > 0


def _write_seq(folder, frames):
    folder.mkdir(parents=True, exist_ok=True)
    paths = []
    for k, f in enumerate(frames):
        p = folder / f"f{k:03d}.png"
        imageio.write_image(p, f)
        paths.append(str(p))
    return paths


def test_seams_on_png_folders(tmp_path, ctx, capsys):
    rng = np.random.default_rng(7)
    xs = _moving(rng, 200, 200, 3, [(0, 0), (2, 1), (4, 2), (6, 3)], block=6)
    ys = _moving(rng, 200, 200, 3, [(0, 0), (-1, 2), (-2, 4), (-3, 6)], block=6)
    px, py = _write_seq(tmp_path / "X", xs), _write_seq(tmp_path / "Y", ys)
    geom = frameflow.flow_geometry(200, 200, 1.0)

    def want(a, b, mode):
        return frameflow.value_of(fnp.pair(fnp.Frame(a, geom, mode == "fisheye_circle"), fnp.Frame(b, geom, mode == "fisheye_circle"))[0])
    assert frameflow._compute_pair_flow_magnitude(px[0], px[1], 1.0) == want(xs[0], xs[1], "none")
    assert frameflow._compute_pair_flow_magnitude(px[0], str(tmp_path / "missing.png"), 1.0) is None
    recs = [{"input_mode": "pair", "file_paths": [px[k], py[k]]} for k in range(4)]
    pair_vals = [(want(xs[k], xs[k + 1], "fisheye_circle") + want(ys[k], ys[k + 1], "fisheye_circle")) / 2.0 for k in range(3)]
    assert frameflow._compute_record_flow_magnitude(recs[0], recs[1], 1.0) == pair_vals[0]
    recs.insert(2, {"input_mode": "pair", "file_paths": [str(tmp_path / "gone.png"), py[0]]})   # breaks the chain
    arr = [0.0] * len(recs)
    n = frameflow._compute_flow_magnitudes(recs, arr, 1.0, 4, "Optical flow")
    # pairs (0,1) and (3,4) (record 2 is missing; records 1 and 3 are not consecutive)
    assert n == 2
    v01 = pair_vals[0]
    v34 = pair_vals[2]
    assert arr == [v01, v01, 0.0, v34, v34]
    assert "Optical flow... 100% (2/2)" in capsys.readouterr().out
