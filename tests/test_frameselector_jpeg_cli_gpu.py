"""-m gpu: the FrameSelector drop-in on folders of JPEG frames, as the GUI runs it (a fresh child process with an argv), once with
GS360_JPEG_DECODER=host and once with device.  The device decoder's gray planes are bit for bit what the passes compute from the host
decoder's RGB frames, so the two CSV files must be byte-identical; the device run says in one [INFO] line what it decoded where."""
import os
import pathlib
import re
import subprocess
import sys

import numpy as np
import pytest

pytest.importorskip("PIL.Image")

import jpegdec_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

CLI = pathlib.Path(__file__).resolve().parents[1] / "360cam-pgm-3dgs-tools_amd" / "cli_tools" / "gs360_FrameSelector.py"
INFO = re.compile(r"^\[INFO\] JPEG decoder: (\d+) frames decoded on the device, (\d+) fallbacks, (\d+) reused$", re.M)


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


def _run(argv, decoder, **env):
    """a fresh child process, as the GUI starts the tool -> its stdout"""
    e = dict(os.environ, GS360_JPEG_DECODER=decoder, **env)
    done = subprocess.run([sys.executable, str(CLI)] + argv, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300, env=e)
    assert done.returncode == 0, done.stdout
    return done.stdout.replace("\r", "\n")


def _both(root, argv, **env):
    """-> (the host run's stdout, the device run's): the same argv with each decoder; the CSV files must be byte-identical"""
    host = _run(["-i", str(root), "-c", "host.csv"] + argv, "host")
    device = _run(["-i", str(root), "-c", "device.csv"] + argv, "device", **env)
    a, b = (root / "host.csv").read_bytes(), (root / "device.csv").read_bytes()
    assert a == b and a.count(b"\n") > 8
    assert not INFO.search(host)
    return host, device


@pytest.fixture(scope="module")
def singles(tmp_path_factory):
    """24 baseline frames (120 x 200, 4:2:0) with a PNG frame, a progressive JPEG and a JPEG cut in the middle of its scan in between"""
    from PIL import Image
    root = tmp_path_factory.mktemp("jpeg_frames")
    frames = _sequence(80, 27, 120, 200)
    for i, f in enumerate(frames):
        if i == 4:
            Image.fromarray(f).save(root / f"frame_{i:04d}.png")
            continue
        data = cases.encode(f, quality=92, subsampling=2, progressive=(i == 11))
        if i == 19:
            from gs360 import jpegdec
            d = jpegdec.parse(data)
            data = data[:d.scan_off + d.scan_len // 2]
        (root / f"frame_{i:04d}.jpg").write_bytes(data)
    return root


def test_hybrid_scores_and_flow_are_byte_identical_and_the_frames_are_decoded_once(singles):
    host, device = _both(singles, ["-d", "--score_backend", "opencv", "-m", "hybrid", "--compute_optical_flow"])
    assert INFO.findall(device) == [("24", "3", "24")]
    assert "Optical flow computed for 26 pair(s):" in device and "Optical flow computed for 26 pair(s):" in host
    rows = (singles / "device.csv").read_text().splitlines()[1:]
    flows = [float(r.split(",")[9]) for r in rows]
    assert any(0.0 < v < 9999.0 for v in flows) and len({r.split(",")[6] for r in rows}) > len(rows) // 2
    strip = lambda out: [ln for ln in out.splitlines() if not INFO.match(ln) and "csv" not in ln]      # noqa: E731
    assert strip(device) == strip(host)                        # nothing else of the output differs


def test_default_backend_is_byte_identical(singles):
    host, device = _both(singles, ["-d"])
    assert INFO.findall(device) == [("24", "3", "0")]


def test_without_a_cache_the_flow_pass_decodes_again(singles):
    host, device = _both(singles, ["-d", "--score_backend", "opencv", "-m", "hybrid", "--compute_optical_flow"], GS360_FS_GRAY_CACHE_MB="0")
    assert INFO.findall(device) == [("24", "3", "0")]


def test_pair_folder_is_byte_identical(tmp_path):
    xs, ys = _sequence(81, 8, 160, 160), _sequence(82, 8, 160, 160)
    for i, (x, y) in enumerate(zip(xs, ys)):
        (tmp_path / f"shot{i:03d}_X.jpg").write_bytes(cases.encode(x, quality=92, subsampling=2))
        (tmp_path / f"shot{i:03d}_Y.jpg").write_bytes(cases.encode(y, quality=92, subsampling=2))
    host, device = _both(tmp_path, ["-d", "-n", "4", "--compute_optical_flow"])
    assert " Input mode pair\n" in device and INFO.findall(device) == [("16", "0", "16")]
