"""cli_tools/gs360_Video2Frames.py end to end on the GPU, its decoder played by tests/fake_ffmpeg_y4m.py (which exits 3 when asked
for a colorspace filter or an RGB format): file names and counts, PNG and TIFF pixels equal to the restatement (16-bit for the 10-bit
clip), JPEG files equal to what the same encoder makes of the restatement's frame, with the host and with the device encoders."""
import io

import numpy as np
import pytest
from PIL import Image

from conftest import ROOT

import gs360_Video2Frames as v2f
import vidcolor_np as ref
from gs360 import imageio, jpegenc

pytestmark = pytest.mark.gpu

FAKE = str(ROOT / "tests" / "fake_ffmpeg_y4m.py")
W, H, N = 70, 34, 6
DEVICE_ENV = {"GS360_JPEG_ENCODER": "device", "GS360_JPEG_HUFFMAN": "optimal", "GS360_PNG_ENCODER": "device"}


def make_clip(path, depth, **extra):
    rng = np.random.default_rng(depth)
    dt = np.uint8 if depth == 8 else np.uint16
    yy, xx = np.mgrid[:H, :W]
    y = np.stack([(16 + (xx * 3 + yy * 2 + 20 * k) % 220) << (depth - 8) for k in range(N)]).astype(dt)
    u, v = (rng.integers(16 << (depth - 8), 240 << (depth - 8), (N, H // 2, W // 2)).astype(dt) for _ in range(2))
    np.savez(path, y=y, u=u, v=v, tag="420jpeg" if depth == 8 else "420p10", **extra)
    return y, u, v


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    d = tmp_path_factory.mktemp("clips")
    out = {}
    for depth in (8, 10):
        out[depth] = (d / f"clip{depth}.npz", make_clip(d / f"clip{depth}.npz", depth))
    return out


def want_frames(clips, depth, keep=False):
    y, u, v = clips[depth][1]
    return [ref.convert(y[k], u[k], v[k], depth, "420", keep_rec709=keep) for k in range(N)]


def run(monkeypatch, capsys, env, *argv):
    for k in DEVICE_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    rc = v2f.run(["--ffmpeg", FAKE, *argv])
    cap = capsys.readouterr()
    return rc, cap.out, cap.err


@pytest.mark.parametrize("env", [{}, DEVICE_ENV], ids=["host", "device"])
def test_png_and_tiff_pixels_are_the_restatements(clips, tmp_path, monkeypatch, capsys, env):
    for depth, ext in ((8, "png"), (10, "png"), (8, "tif")):
        out = tmp_path / f"o{depth}{ext}"
        rc, stdout, stderr = run(monkeypatch, capsys, env, "-i", str(clips[depth][0]), "-f", "1", "-e", ext, "-o", str(out))
        assert rc == 0 and stderr == "" and stdout.rstrip().endswith(f"Completed: {out}"), (stdout, stderr)
        assert "[exec] " in stdout and "yuv4mpegpipe" in stdout
        assert sorted(p.name for p in out.iterdir()) == [f"out_{k:07d}.{ext}" for k in range(N)]
        for k, want in enumerate(want_frames(clips, depth)):
            got = imageio.read_image(out / f"out_{k:07d}.{ext}")
            assert got.dtype == want.dtype and np.array_equal(got, want), (depth, ext, k)


@pytest.mark.parametrize("env", [{}, DEVICE_ENV], ids=["host", "device"])
def test_jpeg_files_are_the_encoders_own_of_the_restatement(clips, ctx, tmp_path, monkeypatch, capsys, env):
    out = tmp_path / "jpg"
    rc, stdout, stderr = run(monkeypatch, capsys, env, "-i", str(clips[8][0]), "-f", "1", "-o", str(out))
    assert rc == 0 and stderr == "", (stdout, stderr)
    assert sorted(p.name for p in out.iterdir()) == [f"out_{k:07d}.jpg" for k in range(N)]
    want = want_frames(clips, 8)
    if env:
        files = jpegenc.encode_device(ctx, want, quality=jpegenc.quality_for(1), restart=jpegenc.RESTART, huffman="optimal")
    else:
        files = []
        for k, rgb in enumerate(want):
            imageio.write_image(tmp_path / f"ref_{k}.jpg", rgb, jpeg_q=1)
            files.append((tmp_path / f"ref_{k}.jpg").read_bytes())
    for k, data in enumerate(files):
        got = np.asarray(Image.open(out / f"out_{k:07d}.jpg").convert("RGB"))
        assert np.array_equal(got, np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))), k
        assert np.abs(got.astype(int) - want[k].astype(int)).max() <= 8       # and it is that picture (quality 100, 4:4:4)


def test_start_end_suffix_and_keep_rec709(clips, tmp_path, monkeypatch, capsys):
    out = tmp_path / "cut"
    rc, stdout, stderr = run(monkeypatch, capsys, {}, "-i", str(clips[8][0]), "-f", "1", "-e", "png", "-o", str(out), "--start", "1", "--end", "4",
                             "--name-suffix", "_L", "--prefix", "cam", "--keep-rec709")
    assert rc == 0 and stderr == "", (stdout, stderr)
    assert sorted(p.name for p in out.iterdir()) == [f"cam_{k:07d}_L.png" for k in range(3)]      # numbered from 0 whatever the cut
    want = want_frames(clips, 8, keep=True)
    for k in range(3):
        assert np.array_equal(imageio.read_image(out / f"cam_{k:07d}_L.png"), want[1 + k])
    assert not np.array_equal(want[1], want_frames(clips, 8)[1])
    # a second run into the same folder is refused, --overwrite replaces
    rc, stdout, stderr = run(monkeypatch, capsys, {}, "-i", str(clips[8][0]), "-f", "0.5", "-e", "png", "-o", str(out), "--name-suffix", "_L", "--prefix", "cam")
    assert rc == 1 and "overwrite is disabled" in stderr
    rc, stdout, stderr = run(monkeypatch, capsys, {}, "-i", str(clips[8][0]), "-f", "0.5", "-e", "png", "-o", str(out), "--name-suffix", "_L", "--prefix", "cam",
                             "--overwrite")
    assert rc == 0 and np.array_equal(imageio.read_image(out / "cam_0000001_L.png"), want_frames(clips, 8)[2])


def test_decoder_failures(clips, tmp_path, monkeypatch, capsys):
    (tmp_path / "broken.npz").write_bytes(b"")
    rc, stdout, stderr = run(monkeypatch, capsys, {}, "-i", str(tmp_path / "broken.npz"), "-f", "1", "-e", "png")
    assert rc == 1 and stderr.strip().splitlines()[-1] == "ffmpeg execution failed (returncode=1)"
    make_clip(tmp_path / "short.npz", 8, cut=5)
    rc, stdout, stderr = run(monkeypatch, capsys, {}, "-i", str(tmp_path / "short.npz"), "-f", "1", "-e", "png")
    lines = stderr.strip().splitlines()
    assert rc == 1 and len(lines) == 1 and lines[0].startswith("[ERR] ") and "truncated" in lines[0]
