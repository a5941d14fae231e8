"""-m gpu: the FrameSelector's three passes on the gray planes of the device JPEG decoder against the same passes on Pillow's RGB
arrays of the same files.  The kernels read a pixel through gray_of<C> and nothing else, and the gray plane holds exactly that
value, so the results must be equal, tuple for tuple and record for record: no tolerance."""
import numpy as np
import pytest

pytest.importorskip("PIL.Image")

import gs360  # noqa: E402
from gs360 import frameflow, framescore, framesource, jpegdec  # noqa: E402

import jpegdec_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = {"q92-420": dict(quality=92, subsampling=2), "q100-444": dict(quality=100, subsampling=0)}


def _sequence(seed, n, H, W):
    """n frames of a drifting blocky texture, each blurred by 0-4 passes of a 3-tap mean and dimmed a little: graded sharpness (the
    texture of tests/test_frameselector_gpu.py, restated)"""
    rng = np.random.default_rng(seed)
    big = np.repeat(np.repeat(rng.integers(0, 256, ((H + 4 * n) // 6 + 2, (W + 4 * n) // 6 + 2, 3)), 6, 0), 6, 1).astype(np.float64)
    big = np.clip(big + rng.integers(-6, 7, big.shape), 0, 255)
    frames = []
    for i in range(n):
        f = big[2 * i:2 * i + H, 3 * i:3 * i + W].copy()
        for _ in range((7 * i) % 5):
            f = (np.roll(f, 1, 0) + f + np.roll(f, -1, 0)) / 3.0
            f = (np.roll(f, 1, 1) + f + np.roll(f, -1, 1)) / 3.0
        frames.append(np.clip(f * (0.35 + 0.65 * ((11 * i) % 7) / 6.0), 0, 255).astype(np.uint8))
    return frames


@pytest.fixture(scope="module")
def ctx():
    with gs360.Context(device=0, n_slots=1) as c:
        yield c


@pytest.fixture(scope="module")
def sets(ctx):
    """{(kind, shape name): (Pillow's RGB arrays, DeviceFrames of the gray decode)} for 12 singles of 120 x 200 and 8 pair-sized
    frames of 160 x 160 per kind, decoded once"""
    out, bufs = {}, []
    for kind, kw in KINDS.items():
        for name, frames in (("single", _sequence(70, 12, 120, 200)), ("pair", _sequence(71, 8, 160, 160))):
            datas = [cases.encode(f, **kw) for f in frames]
            host = [cases.pillow(d) for d in datas]
            dev = []
            for r in jpegdec.decode_device(ctx, datas, gray=True):
                assert r.status == 0 and r.shape == host[0].shape[:2] + (1,)
                bufs.append(r.buf)
                dev.append(framescore.DeviceFrame(r.buf, r.shape[0], r.shape[1], 1, r.stride))
            out[kind, name] = (host, dev)
    yield out
    for b in bufs:
        ctx.free(b)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fft", framescore.FFT_MODES)
@pytest.mark.parametrize("metric", ("lapvar", "fft", "hybrid"))
def test_scores_on_gray_planes_equal_scores_on_rgb(ctx, sets, metric, fft, kind):
    for name, mask_mode, crop in (("single", "none", 0.8), ("pair", "fisheye_circle", 1.0), ("single", "fisheye_circle", 0.8)):
        host, dev = sets[kind, name]
        for ignore_highlights in (True, False):
            want = framescore.score_arrays(ctx, host, metric, crop, True, ignore_highlights, mask_mode, fft=fft)
            got = framescore.score_arrays(ctx, dev, metric, crop, True, ignore_highlights, mask_mode, fft=fft)
            assert got == want, (name, mask_mode, ignore_highlights)
            assert all(t[0] is not None for t in want)
            if mask_mode == "none":
                assert len({t[0] for t in want}) > len(want) // 2                 # graded, not constant


@pytest.mark.parametrize("kind", KINDS)
def test_edge_scores_on_gray_planes_equal_those_on_rgb(ctx, sets, kind):
    host, dev = sets[kind, "single"]
    want = framescore.edge_arrays(ctx, host, 0.8)
    assert framescore.edge_arrays(ctx, dev, 0.8) == want
    assert len({t[0] for t in want}) > len(want) // 2


@pytest.mark.parametrize("kind", KINDS)
def test_flow_records_on_gray_planes_equal_those_on_rgb(ctx, sets, kind):
    for name, mask_mode, crop in (("single", "none", frameflow.FLOW_CROP_RATIO), ("pair", "fisheye_circle", 1.0)):
        host, dev = sets[kind, name]
        pairs = [(k, k + 1) for k in range(len(host) - 1)]
        want = frameflow.flow_records(ctx, host, pairs, crop, mask_mode)
        got = frameflow.flow_records(ctx, dev, pairs, crop, mask_mode)
        assert got.tobytes() == want.tobytes(), (name, got, want)
        assert any(r["n_tracked"] > 0 for r in want)
        # a gray plane beside a host frame (a file the device decoder left to the host): the pair is computed from both grays
        mixed = [dev[k] if k % 2 else host[k] for k in range(len(host))]
        assert frameflow.flow_records(ctx, mixed, pairs, crop, mask_mode).tobytes() == want.tobytes(), name


def test_reader_scores_files_like_the_host_path(ctx, tmp_path, monkeypatch):
    """score_files and the flow pass through framesource (a store open) against the host decoder, on files: baseline frames with a
    PNG, a progressive file and a cut one in between"""
    from PIL import Image
    frames = _sequence(72, 10, 120, 200)
    paths = []
    for i, f in enumerate(frames):
        p = tmp_path / (f"f{i:02d}.png" if i == 3 else f"f{i:02d}.jpg")
        if i == 3:
            Image.fromarray(f).save(p)
        else:
            data = cases.encode(f, quality=92, subsampling=2, progressive=(i == 5))
            p.write_bytes(data[:len(data) // 2] if i == 7 else data)
        paths.append(str(p))
    monkeypatch.setattr(framescore, "default_context", lambda: ctx)
    records = [{"file_paths": [p]} for p in paths]

    def both():
        tuples = framescore.score_files(paths, "hybrid", 0.8, 0, False, True, workers=4)
        mags = [0.0] * len(paths)
        done = frameflow._compute_flow_magnitudes(records, mags, frameflow.FLOW_CROP_RATIO, 4, "Optical flow")
        return tuples, mags, done
    monkeypatch.delenv("GS360_JPEG_DECODER", raising=False)
    want = both()
    monkeypatch.setenv("GS360_JPEG_DECODER", "device")
    with framesource.open_store():
        got = both()
        st = framesource.stats()
        assert (st["device_decoded"], st["fallbacks"], st["reused"]) == (7, 3, 7) and st["kept_bytes"] == 7 * 120 * 200
    assert got == want and want[2] == 9 and any(0.0 < m < 9999.0 for m in want[1])
    assert framesource.stats()["kept_bytes"] == 0
    # without a store every call frees what it decoded, and the single-file seams take the same path
    assert framescore.score_one_file(paths[0], "hybrid", 0.8, 0, False, True) == want[0][0]
    assert framescore.score_one_file_ffmpeg(paths[1], "hybrid", 0.8, 0, False, True) == framescore.edge_arrays(ctx, [cases.pillow(open(paths[1], "rb").read())], 0.8)[0]
    monkeypatch.delenv("GS360_JPEG_DECODER")
    pair_host = frameflow._compute_pair_flow_magnitude(paths[0], paths[1], frameflow.FLOW_CROP_RATIO)
    monkeypatch.setenv("GS360_JPEG_DECODER", "device")
    assert frameflow._compute_pair_flow_magnitude(paths[0], paths[1], frameflow.FLOW_CROP_RATIO) == pair_host
