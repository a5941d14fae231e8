"""gs360_frame_fft_energy on the MI355X (FS-FFT v1): records against the float64 restatement (tests/framescore_fft_np.py) and the
reference's complex64 fft_energy within the stated bound, bit-identical repeats, batches split at GS360_MAX_FRAMES, argument
checks, and score_arrays(fft="device") against fft="host"."""
import numpy as np
import pytest

import framescore_fft_np as ffnp
from gs360 import capi, framescore

pytestmark = pytest.mark.gpu

REL, ABS = 1e-5, 1e-3          # DESIGN.md FS-FFT v1: |dev - ref| <= REL * ref + ABS on the energy (a mean of |S|)
FLAGS = [0, capi.FS_CIRCLE, capi.FS_HIGHLIGHTS, capi.FS_CIRCLE | capi.FS_HIGHLIGHTS]
SIZES = [(204, 512), (409, 512), (512, 512), (509, 127), (127, 509), (1, 512), (512, 1), (1, 1), (17, 3), (3, 17)]   # h, w


def _planes(rng, h, w, kind):
    yy, xx = np.mgrid[:h, :w]
    if kind == "constant":
        g = np.full((h, w), 181.625, np.float32)
    elif kind == "noise":
        g = rng.uniform(0, 255, size=(h, w)).astype(np.float32)
    else:   # photo-like: gradients, an edge, a bright disc, mild noise
        g = 60 + 0.3 * xx + 0.2 * yy + np.where(xx > w / 2, 70, 0) + rng.normal(0, 2, size=(h, w))
        g = np.where((xx - w / 3) ** 2 + (yy - h / 2) ** 2 < (min(h, w) / 4) ** 2, 250, g)
        g = np.clip(g, 0, 255).astype(np.float32)
    near = np.clip(np.round(g + rng.integers(-2, 3, size=(h, w))), 0, 255).astype(np.float32)
    return g, near


def _geometry(h, w):
    H, W = 2 * h + 3, 3 * w + 1
    return H, W, framescore.band_rows(H, 0.8)


def _run(ctx, planes, H, W, band, flags):
    h, w = planes[0][0].shape
    bufs = [ctx.to_device(np.stack(p)) for p in planes]
    out = ctx.alloc(len(planes) * framescore.FFT_DTYPE.itemsize)
    try:
        ctx.frame_fft_energy_dev(bufs, w, h, H, W, band, out, flags=flags)
        recs = ctx.download(out, (len(planes),), framescore.FFT_DTYPE)
    finally:
        for b in bufs + [out]:
            ctx.free(b)
    return [{f: r[f].item() for f in framescore.FFT_DTYPE.names} for r in recs]


def _within(got, want):
    return abs(got - want) <= REL * abs(want) + ABS


def _check(rec, g, near, H, W, band, flags):
    h, w = g.shape
    ref = ffnp.fft_record(g, near, H, W, band, flags)
    assert rec["n"] == ref["n"] == h * w and rec["n_valid"] == ref["n_valid"]
    mask = ffnp.geometry(h, w, H, W, band, flags, near)[1].astype(np.uint8)
    for masked in (False, True):
        got = framescore.fft_energy_from_record(rec, masked)
        f64 = framescore.fft_energy_from_record(ref, masked)
        c64 = framescore.fft_energy(g, mask if masked else None)
        assert _within(got, f64), (masked, got, f64)
        assert _within(got, c64), (masked, got, c64)


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("kind", ["constant", "noise", "photo"])
@pytest.mark.parametrize("flags", FLAGS)
def test_records_within_the_bound(ctx, h, w, kind, flags):
    rng = np.random.default_rng(h * 1000 + w)
    g, near = _planes(rng, h, w, kind)
    H, W, band = _geometry(h, w)
    rec = _run(ctx, [(g, near)], H, W, band, flags)[0]
    _check(rec, g, near, H, W, band, flags)
    if kind == "constant":       # the DC term does not leak into the donut
        assert rec["sum_hf"] / rec["n"] < 1e-3


def test_empty_valid_mask_and_all_highlights(ctx):
    rng = np.random.default_rng(3)
    g, _ = _planes(rng, 204, 512, "photo")
    near = np.full_like(g, 250.0)
    H, W, band = 3840, 7680, framescore.band_rows(3840, 0.8)
    for flags in (capi.FS_HIGHLIGHTS, capi.FS_CIRCLE | capi.FS_HIGHLIGHTS):
        rec = _run(ctx, [(g, near)], H, W, band, flags)[0]
        assert rec["n_valid"] == 0 and rec["sum_hf_valid"] == 0.0
        _check(rec, g, near, H, W, band, flags)


@pytest.mark.parametrize("n", [1, 16, 17, 35])
def test_batches_and_repeats_are_bit_identical(ctx, n):
    rng = np.random.default_rng(100 + n)
    h, w = 204, 512
    H, W, band = 3840, 7680, framescore.band_rows(3840, 0.8)
    planes = [_planes(rng, h, w, ("noise", "photo", "constant")[k % 3]) for k in range(n)]
    flags = capi.FS_CIRCLE | capi.FS_HIGHLIGHTS
    a = _run(ctx, planes, H, W, band, flags)
    b = _run(ctx, planes, H, W, band, flags)
    assert a == b
    for k in range(n):
        _check(a[k], *planes[k], H, W, band, flags)
    for k in (0, n - 1):            # a frame's record does not depend on its batch
        assert _run(ctx, [planes[k]], H, W, band, flags)[0] == a[k]


def test_argument_errors(ctx):
    buf = ctx.alloc(2 * 64 * 64 * 4)
    out = ctx.alloc(32)
    try:
        def call(small_w=64, small_h=64, H=100, W=100, band=(0, 100), flags=0, bufs=(buf,)):
            ctx.frame_fft_energy_dev(list(bufs), small_w, small_h, H, W, band, out, flags=flags)
        call()
        ctx.sync(0)
        for kw in ({"small_w": 0}, {"small_h": 0}, {"small_w": 513, "W": 2000}, {"small_h": 513, "H": 2000, "band": (0, 2000)},
                   {"small_w": 101}, {"small_h": 60, "band": (10, 60)}, {"flags": 4}, {"band": (50, 40)}, {"H": 0}):
            with pytest.raises(capi.Gs360Error) as e:
                call(**kw)
            assert e.value.code == -1, kw
        null = type("Null", (), {"ptr": None})()
        with pytest.raises(capi.Gs360Error) as e:
            call(bufs=(buf, null))
        assert e.value.code == -1
    finally:
        ctx.free(buf)
        ctx.free(out)


def _frame(rng, H, W, C):
    yy, xx = np.mgrid[:H, :W]
    g = (xx * 7 + yy * 3) % 256
    g = np.where((xx - W / 3) ** 2 + (yy - H / 2) ** 2 < (min(H, W) / 4) ** 2, 250, g)
    g = np.clip(g + rng.integers(-3, 4, size=g.shape), 0, 255).astype(np.uint8)
    return g if C == 1 else np.repeat(g[:, :, None], C, axis=2) ^ np.arange(C, dtype=np.uint8) * 17


def _assert_same_scores(dev, host):
    assert len(dev) == len(host)
    for d, h in zip(dev, host):
        for k, (a, b) in enumerate(zip(d, h)):
            if k in (0, 7) and a is not None:
                assert _within(a, b), (k, a, b)
            else:
                assert a == b, k


SCORE_CASES = [  # H, W, C, red_index, mask_mode, ignore_highlights, n frames
    (300, 700, 3, 0, "none", True, 3), (300, 700, 3, 2, "none", False, 2), (257, 513, 1, 0, "none", True, 2),
    (240, 240, 4, 0, "fisheye_circle", True, 2), (3840, 3840, 3, 0, "fisheye_circle", True, 2), (3840, 7680, 3, 0, "none", True, 2)]


@pytest.mark.parametrize("H,W,C,red,mask_mode,hl,n", SCORE_CASES)
@pytest.mark.parametrize("metric", framescore.METRICS)
def test_score_arrays_device_equals_host(ctx, H, W, C, red, mask_mode, hl, n, metric):
    rng = np.random.default_rng(H + W + C)
    frames = [_frame(rng, H, W, C) for _ in range(n)]
    if n > 2:
        frames[-1] = np.full_like(frames[-1], 255)      # all highlight
    host = framescore.score_arrays(ctx, frames, metric, 0.8, True, hl, mask_mode, red_index=red, fft="host")
    dev = framescore.score_arrays(ctx, frames, metric, 0.8, True, hl, mask_mode, red_index=red, fft="device")
    _assert_same_scores(dev, host)


def test_device_frames_download_two_records_per_batch(ctx, monkeypatch):
    rng = np.random.default_rng(11)
    imgs = [_frame(rng, 200, 640, 3) for _ in range(17)]
    bufs = [ctx.to_device(a) for a in imgs]
    calls = []
    real = ctx.download

    def download(buf, shape, dtype=np.uint8, slot=0):
        out = real(buf, shape, dtype, slot)
        calls.append(out.nbytes)
        return out
    try:
        frames = [framescore.DeviceFrame(b, 200, 640, 3) for b in bufs]
        monkeypatch.setattr(ctx, "download", download)
        dev = framescore.score_arrays(ctx, frames, "hybrid", 0.8, True, True, fft="device")
        monkeypatch.undo()
    finally:
        for b in bufs:
            ctx.free(b)
    assert calls == [16 * 104, 16 * 32, 1 * 104, 1 * 32]       # the stats and fft records of each batch, no plane
    _assert_same_scores(dev, framescore.score_arrays(ctx, imgs, "hybrid", 0.8, True, True, fft="host"))
