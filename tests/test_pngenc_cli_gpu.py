"""-m gpu: GS360_PNG_ENCODER=device through the drop-ins.  gs360_360PerspCut --ext png on an 8-bit and on a 16-bit panorama and the
dual-fisheye tool with masks: with the variable set every .png decodes to exactly the pixels of the run without it, under the same file
names, log lines and exit code, and is the NumPy restatement of PNG-SPEC v1 (tests/pngenc_np.py) of those pixels; with it unset the
files are the host writers', as before."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gs360_360PerspCut as cut
from conftest import PKG
from gs360 import imageio

import pngenc_cases as cases
import pngenc_np as ref
from test_dualfisheye_cli import SMALL_XML, make_pairs

pytestmark = pytest.mark.gpu
CUT = [sys.executable, str(PKG / "cli_tools" / "gs360_360PerspCut.py")]
DUAL = [sys.executable, str(PKG / "cli_tools" / "gs360_DualFisheyeDistortionCalibration.py")]


def run_cli(exe, args, out, encoder):
    """-> stdout with the run's own output folder replaced by OUT"""
    env = {k: v for k, v in os.environ.items() if k != "GS360_PNG_ENCODER"}
    if encoder:
        env["GS360_PNG_ENCODER"] = encoder
    r = subprocess.run(exe + args, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.replace(str(out), "OUT")


def files_of(out):
    return {str(p.relative_to(out)): p for p in sorted(out.rglob("*.png"))}


def same_pixels_new_bytes(host, dev, dtype):
    """the device run's files: the host run's names and pixels, the restatement's bytes"""
    a, b = files_of(host), files_of(dev)
    assert sorted(a) == sorted(b) and a
    for name in a:
        want, got = imageio.read_image(a[name]), imageio.read_image(b[name])
        assert want.dtype == got.dtype == dtype and np.array_equal(want, got), name
        assert b[name].read_bytes() == ref.encode(want), name
    return a


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_perspcut_png_views(tmp_path, dtype, monkeypatch):
    src = tmp_path / "in"
    src.mkdir()
    imageio.write_image(src / "pano.png", cases._photo(64, 128, 3, dtype, 31))
    base = ["-i", str(src), "--count", "3", "--size", "32", "--ext", "png"]
    host, dev = tmp_path / "host", tmp_path / "dev"
    log_host = run_cli(CUT, base + ["-o", str(host)], host, None)
    log_dev = run_cli(CUT, base + ["-o", str(dev)], dev, "device")
    assert log_host == log_dev and "failed=0" in log_dev
    names = same_pixels_new_bytes(host, dev, dtype)
    assert len(names) == 3
    path = tmp_path / "again.png"                                                  # the variable unset: the host writer's bytes
    imageio.write_image(path, imageio.read_image(names[sorted(names)[0]]))
    assert names[sorted(names)[0]].read_bytes() == path.read_bytes()
    # the engine's counters, in process: one device file per view
    from gs360 import engine
    args = cut.create_arg_parser().parse_args(base + ["-o", str(tmp_path / "inproc")])
    for attr in ("size", "hfov", "focal_mm"):
        setattr(args, f"{attr}_explicit", getattr(args, f"{attr}_explicit", False))
    args.input_is_video, args.video_bit_depth = False, 8
    (tmp_path / "inproc").mkdir()
    jobs = cut.build_view_jobs(args, [src / "pano.png"], tmp_path / "inproc").jobs
    cut.stop_event.clear()
    monkeypatch.setenv("GS360_PNG_ENCODER", "device")
    before = engine.get_engine().stats()
    assert [cut.run_one(cmd) for cmd, _s, _d in jobs] == [(0, "")] * 3
    after = engine.get_engine().stats()
    written = files_of(tmp_path / "inproc")
    assert sorted(written) == sorted(names)
    assert after["png_device_images"] - before["png_device_images"] == 3
    assert after["png_device_bytes"] - before["png_device_bytes"] == sum(p.stat().st_size for p in written.values())
    for name, p in written.items():
        assert p.read_bytes() == (dev / name).read_bytes(), name


def test_dual_fisheye_png_views_and_masks(tmp_path):
    shots, masks = tmp_path / "shots", tmp_path / "masks"
    make_pairs(shots, n=1)
    masks.mkdir()
    rng = np.random.default_rng(9)
    for p in sorted(shots.glob("frame_*.png")):
        imageio.write_image(masks / p.name, (rng.random((240, 240)) > 0.3).astype(np.uint8) * 255)
    xml = tmp_path / "c.xml"
    xml.write_text(SMALL_XML)
    args = ["-i", str(shots), "-x", str(xml), "--interpolation", "linear", "--perspective-size", "64", "--perspective-ext", "png",
            "--workers", "2", "--mask-value", "5", "--map-mode", "table", "--mask-input-dir", str(masks)]
    host, dev = tmp_path / "host", tmp_path / "dev"
    log_host = run_cli(DUAL, args + ["--perspective-output-dir", str(host)], host, None)
    log_dev = run_cli(DUAL, args + ["--perspective-output-dir", str(dev)], dev, "device")
    assert log_host == log_dev and "errors=0" in log_dev
    names = same_pixels_new_bytes(host, dev, np.uint8)
    assert sum(n.startswith("Masks/") for n in names) == 10 and sum(n.startswith("Images/") for n in names) == 10
