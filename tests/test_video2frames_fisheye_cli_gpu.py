"""cli_tools/gs360_Video2Frames.py --fisheye-perspective end to end on the GPU under GS360_V2F_FISHEYE=device, its decoder played by
tests/fake_ffmpeg_y4m.py (which refuses any command line but the plain Y4M decode): file names and counts, PNG and TIFF pixels equal
to tests/vidfisheye_np.py's view (16-bit for the 10-bit clip), JPEG files equal to what the same encoder makes of that view, with the
host and with the device encoders, both projections, --keep-rec709, and an unknown value of the variable."""
import io

import numpy as np
import pytest
from PIL import Image

from conftest import ROOT

import gs360_Video2Frames as v2f
import vidfisheye_np as ref
from gs360 import imageio, jpegenc

pytestmark = pytest.mark.gpu

FAKE = str(ROOT / "tests" / "fake_ffmpeg_y4m.py")
W, H, N, S = 70, 34, 3, 40
DEVICE_ENV = {"GS360_JPEG_ENCODER": "device", "GS360_JPEG_HUFFMAN": "optimal", "GS360_PNG_ENCODER": "device"}
ON = {"GS360_V2F_FISHEYE": "device"}
GEOMETRY = ref.geometry(8.0, S, 180.0)          # the tool's defaults: an 8 mm lens, a 180 degree circle


def make_clip(path, depth):
    rng = np.random.default_rng(190 + depth)
    dt = np.uint8 if depth == 8 else np.uint16
    yy, xx = np.mgrid[:H, :W]
    y = np.stack([(16 + (xx * 3 + yy * 2 + 20 * k) % 220) << (depth - 8) for k in range(N)]).astype(dt)
    u, v = (rng.integers(16 << (depth - 8), 240 << (depth - 8), (N, H // 2, W // 2)).astype(dt) for _ in range(2))
    np.savez(path, y=y, u=u, v=v, tag="420jpeg" if depth == 8 else "420p10")
    return y, u, v


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    d = tmp_path_factory.mktemp("clips")
    return {depth: (d / f"clip{depth}.npz", make_clip(d / f"clip{depth}.npz", depth)) for depth in (8, 10)}


def want_frames(clips, depth, projection, keep=False):
    y, u, v = clips[depth][1]
    return [ref.render(y[k], u[k], v[k], depth, "420", projection, S, *GEOMETRY, keep_rec709=keep) for k in range(N)]


def run(monkeypatch, capsys, env, *argv):
    for k in list(DEVICE_ENV) + list(ON):
        monkeypatch.delenv(k, raising=False)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    rc = v2f.run(["--ffmpeg", FAKE, "--fisheye-perspective", "--fisheye-size", str(S), *argv])
    cap = capsys.readouterr()
    return rc, cap.out, cap.err


@pytest.mark.parametrize("env", [{}, DEVICE_ENV], ids=["host", "device"])
@pytest.mark.parametrize("projection", ["equidistant", "equisolid"])
def test_png_and_tiff_pixels_are_the_restatements(clips, tmp_path, monkeypatch, capsys, projection, env):
    for depth, ext in ((8, "png"), (10, "png"), (8, "tif")):
        out = tmp_path / f"o{depth}{ext}"
        rc, stdout, stderr = run(monkeypatch, capsys, dict(env, **ON), "-i", str(clips[depth][0]), "-f", "1", "-e", ext, "-o", str(out),
                                 "--fisheye-projection", projection)
        assert rc == 0 and stderr == "" and stdout.rstrip().endswith(f"Completed: {out}"), (stdout, stderr)
        assert "[exec] " in stdout and "yuv4mpegpipe" in stdout and "v360" not in stdout and f"[progress] frame {N}" in stdout
        assert sorted(p.name for p in out.iterdir()) == [f"out_{k:07d}.{ext}" for k in range(N)]
        for k, want in enumerate(want_frames(clips, depth, projection)):
            got = imageio.read_image(out / f"out_{k:07d}.{ext}")
            assert got.shape == (S, S, 3) and got.dtype == want.dtype and np.array_equal(got, want), (depth, ext, k)
            assert want.any()


@pytest.mark.parametrize("env", [{}, DEVICE_ENV], ids=["host", "device"])
def test_jpeg_files_are_the_encoders_own_of_the_restatement(clips, ctx, tmp_path, monkeypatch, capsys, env):
    out = tmp_path / "jpg"
    rc, stdout, stderr = run(monkeypatch, capsys, dict(env, **ON), "-i", str(clips[8][0]), "-f", "1", "-o", str(out))
    assert rc == 0 and stderr == "", (stdout, stderr)
    assert sorted(p.name for p in out.iterdir()) == [f"out_{k:07d}.jpg" for k in range(N)]
    want = want_frames(clips, 8, "equisolid")                  # the tool's default projection
    if env:
        files = jpegenc.encode_device(ctx, want, quality=jpegenc.quality_for(1), restart=jpegenc.RESTART, huffman="optimal")
    else:
        files = []
        for k, rgb in enumerate(want):
            imageio.write_image(tmp_path / f"ref_{k}.jpg", rgb, jpeg_q=1)
            files.append((tmp_path / f"ref_{k}.jpg").read_bytes())
    for k, data in enumerate(files):
        got = np.asarray(Image.open(out / f"out_{k:07d}.jpg").convert("RGB"))
        assert got.shape == (S, S, 3) and np.array_equal(got, np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))), k


def test_keep_rec709_suffix_and_cut(clips, tmp_path, monkeypatch, capsys):
    out = tmp_path / "cut"
    rc, stdout, stderr = run(monkeypatch, capsys, ON, "-i", str(clips[8][0]), "-f", "1", "-e", "png", "-o", str(out), "--start", "1",
                             "--name-suffix", "_L", "--prefix", "cam", "--keep-rec709")
    assert rc == 0 and stderr == "", (stdout, stderr)
    assert sorted(p.name for p in out.iterdir()) == [f"cam_{k:07d}_L.png" for k in range(N - 1)]
    want = want_frames(clips, 8, "equisolid", keep=True)
    for k in range(N - 1):
        assert np.array_equal(imageio.read_image(out / f"cam_{k:07d}_L.png"), want[1 + k])
    assert not np.array_equal(want[1], want_frames(clips, 8, "equisolid")[1])


def test_an_unknown_value_of_the_variable(clips, tmp_path, monkeypatch, capsys):
    out = tmp_path / "none"
    rc, stdout, stderr = run(monkeypatch, capsys, {"GS360_V2F_FISHEYE": "host"}, "-i", str(clips[8][0]), "-f", "1", "-e", "png", "-o", str(out))
    lines = stderr.strip().splitlines()
    assert rc == 1 and len(lines) == 1 and lines[0].startswith("[ERR] ") and "GS360_V2F_FISHEYE" in lines[0]
    assert not out.exists()
    # the argument checks come first, with the reference's messages
    rc, stdout, stderr = run(monkeypatch, capsys, ON, "-i", str(clips[8][0]), "-f", "1", "--fisheye-focal-mm", "0")
    assert rc == 1 and stderr.strip() == "Focal length must be greater than zero when using --fisheye-perspective."
    # and without the variable the flag is refused as before
    rc, stdout, stderr = run(monkeypatch, capsys, {}, "-i", str(clips[8][0]), "-f", "1", "-e", "png", "-o", str(out))
    assert rc == 1 and "--fisheye-perspective is not implemented" in stderr and not out.exists()
