"""gs360_frame_flow_u8 on the MI355X against the FS-FLOW v1 restatement (tests/frameflow_np.py), exactly: every corner in order,
every point's status and float32 end position, and every record; then the drop-in seams of gs360.frameflow on PNG folders."""
import numpy as np
import pytest

import frameflow_np as fnp
from gs360 import framescore, frameflow, imageio

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


def _check(ctx, frames, pairs, crop, mode, red_index=0, dev_frames=None):
    recs, pts = frameflow.flow_records(ctx, dev_frames or frames, pairs, crop, mode, red_index, with_points=True)
    H, W = frames[0].shape[:2]
    geom = frameflow.flow_geometry(H, W, crop)
    cache = {}
    for k, (a, b) in enumerate(pairs):
        for f in (a, b):
            if f not in cache:
                cache[f] = fnp.Frame(frames[f], geom, mode == "fisheye_circle", red_index)
        (nc, nt, s), p0, p1, st = fnp.pair(cache[a], cache[b])
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
