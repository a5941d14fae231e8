"""-m gpu: GS360_JPEG_HUFFMAN=optimal through the gs360_360PerspCut drop-in.  With GS360_JPEG_ENCODER=device and the switch on, every
.jpg the CLI writes must be the restatement of "JPG-SPEC v1, optimal tables" (tests/jpegopt_np.py) applied to the pixels the same command
writes as PNG; with the encoder alone the files are the standard-table ones, with neither variable Pillow's, as before."""
import io
import os
import stat
import subprocess
import sys

import numpy as np
import pytest

import gs360_360PerspCut as cut
from conftest import PKG, ROOT
from gs360 import imageio

import jpegenc_np as ref
import jpegopt_np as opt

pytestmark = pytest.mark.gpu
EXE = [sys.executable, str(PKG / "cli_tools" / "gs360_360PerspCut.py")]
FAKE = ROOT / "tests" / "fake_ffmpeg.py"
VARS = ("GS360_JPEG_ENCODER", "GS360_JPEG_OPTIMIZE", "GS360_JPEG_HUFFMAN")


def run_cli(args, encoder, huffman=None):
    env = {k: v for k, v in os.environ.items() if k not in VARS}
    if encoder:
        env["GS360_JPEG_ENCODER"] = encoder
    if huffman:
        env["GS360_JPEG_HUFFMAN"] = huffman
    r = subprocess.run(EXE + args, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "failed=0" in r.stdout, r.stdout + r.stderr


def test_cli_still_images_optimal_standard_and_default(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    src = tmp_path / "in"
    src.mkdir()
    imageio.write_image(src / "pano.png", ref.photo_image(64, 128))
    base = ["-i", str(src), "--count", "2", "--size", "32"]
    run_cli(base + ["--ext", "png", "-o", str(tmp_path / "png")], None)
    run_cli(base + ["-o", str(tmp_path / "opt100")], "device", "optimal")
    run_cli(base + ["-o", str(tmp_path / "opt95"), "--jpeg-quality-95"], "device", "optimal")
    run_cli(base + ["-o", str(tmp_path / "dev")], "device")
    run_cli(base + ["-o", str(tmp_path / "host")], None)
    pngs = sorted((tmp_path / "png").glob("*.png"))
    assert len(pngs) == 2
    for p in pngs:
        pixels = imageio.read_image(p)
        assert pixels.shape == (32, 32, 3)
        std = ref.encode(pixels, 100, 8)
        for folder, quality in (("opt100", 100), ("opt95", 95)):
            got = (tmp_path / folder / (p.stem + ".jpg")).read_bytes()
            assert got == opt.encode_optimal(pixels, quality, 8), (folder, p.name)
            assert np.asarray(Image.open(io.BytesIO(got))).shape == (32, 32, 3)
        assert len((tmp_path / "opt100" / (p.stem + ".jpg")).read_bytes()) < len(std)
        assert (tmp_path / "dev" / (p.stem + ".jpg")).read_bytes() == std, p.name              # the encoder alone: standard tables
        b = io.BytesIO()
        Image.fromarray(pixels).save(b, "JPEG", quality=100, subsampling=0, optimize=True)
        assert (tmp_path / "host" / (p.stem + ".jpg")).read_bytes() == b.getvalue(), p.name    # neither variable: Pillow's bytes


def plan_video_jobs(tmp_path, out, extra):
    prog = tmp_path / "ffmpeg_double"
    prog.write_text("#!/bin/sh\nexec {} {} \"$@\"\n".format(sys.executable, FAKE))
    prog.chmod(prog.stat().st_mode | stat.S_IXUSR)
    args = cut.create_arg_parser().parse_args(["-i", str(tmp_path / "clip.npy"), "--ffmpeg", str(prog), "-f", "1", "--count", "2",
                                               "--size", "32"] + extra)
    for attr in ("size", "hfov", "focal_mm"):
        setattr(args, f"{attr}_explicit", getattr(args, f"{attr}_explicit", False))
    args.input_is_video, args.video_bit_depth = True, 8
    out.mkdir()
    return cut.build_view_jobs(args, [tmp_path / "clip.npy"], out)


def test_video_frames_through_the_decoder_double(tmp_path, monkeypatch):
    from concurrent.futures import ThreadPoolExecutor
    from gs360 import engine
    rng = np.random.default_rng(43)
    np.save(tmp_path / "clip.npy", rng.integers(0, 256, (3, 64, 128, 3), dtype=np.uint8))
    cut.stop_event.clear()
    for v in VARS:
        monkeypatch.delenv(v, raising=False)
    png = plan_video_jobs(tmp_path, tmp_path / "png", ["--ext", "png"])
    with ThreadPoolExecutor(max_workers=2) as pool:
        assert list(pool.map(cut.run_one, [cmd for cmd, _s, _d in png.jobs])) == [(0, "")] * 2
    before = engine.get_engine().stats()
    monkeypatch.setenv("GS360_JPEG_ENCODER", "device")
    monkeypatch.setenv("GS360_JPEG_HUFFMAN", "optimal")
    jpg = plan_video_jobs(tmp_path, tmp_path / "jpg", [])
    with ThreadPoolExecutor(max_workers=2) as pool:
        assert list(pool.map(cut.run_one, [cmd for cmd, _s, _d in jpg.jobs])) == [(0, "")] * 2
    after = engine.get_engine().stats()
    assert {k for k in after if "jpeg" in k} == {"jpeg_device_images", "jpeg_device_bytes"}      # the mode adds no key to the statistics
    pngs = sorted((tmp_path / "png").glob("*.png"))
    assert len(pngs) == 6                                              # 3 frames x 2 views
    total = 0
    for p in pngs:
        got = (tmp_path / "jpg" / (p.stem + ".jpg")).read_bytes()
        assert got == opt.encode_optimal(imageio.read_image(p), 100, 8), p.name
        total += len(got)
    assert after["jpeg_device_images"] - before["jpeg_device_images"] == 6
    assert after["jpeg_device_bytes"] - before["jpeg_device_bytes"] == total
