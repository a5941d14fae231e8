"""-m gpu: GS360_JPEG_DECODER=device through the two drop-in tools.  The views are written as PNG, so the comparison is of pixels: a run
with the device decoder writes byte for byte the files of the host decoder's run, a folder with a progressive JPEG and a PNG in it as
well (those take the host path), and the engine's counter shows that the baseline files were decoded on the device."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

pytest.importorskip("PIL.Image")
from PIL import Image  # noqa: E402

import gs360_360PerspCut as cut  # noqa: E402
from conftest import PKG  # noqa: E402
from test_dualfisheye_cli import SMALL_XML  # noqa: E402

pytestmark = pytest.mark.gpu
CUT = [sys.executable, str(PKG / "cli_tools" / "gs360_360PerspCut.py")]
DF = [sys.executable, str(PKG / "cli_tools" / "gs360_DualFisheyeDistortionCalibration.py")]


def run(cmd, decoder, ok):
    env = {k: v for k, v in os.environ.items() if k != "GS360_JPEG_DECODER"}
    if decoder:
        env["GS360_JPEG_DECODER"] = decoder
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and ok in r.stdout, r.stdout + r.stderr
    return r.stdout


def photo(h, w, seed):
    """smooth structure plus noise: every coefficient class occurs"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    base = np.stack([128 + 100 * np.sin(xx / 17.0 + seed), 128 + 100 * np.cos(yy / 11.0), (xx * 3 + yy * 5) % 256], -1)
    return np.clip(base + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)


def files_of(out, pattern="*.png"):
    return {str(p.relative_to(out)): p.read_bytes() for p in sorted(out.rglob(pattern)) if p.is_file()}


@pytest.fixture(scope="module")
def panos(tmp_path_factory):
    root = tmp_path_factory.mktemp("jpd_cut")
    plain, mixed = root / "plain", root / "mixed"
    for d in (plain, mixed):
        d.mkdir()
    Image.fromarray(photo(256, 512, 1)).save(plain / "a.jpg", quality=92)                               # 4:2:0, Pillow's default
    Image.fromarray(photo(256, 512, 2)).save(plain / "b.jpg", quality=95, subsampling=0)
    Image.fromarray(photo(256, 512, 3)).save(plain / "c.jpeg", quality=85, restart_marker_blocks=16)
    Image.fromarray(photo(256, 512, 4)).save(mixed / "prog.jpg", quality=90, progressive=True)
    Image.fromarray(photo(256, 512, 5)).save(mixed / "lossless.png")
    Image.fromarray(photo(256, 512, 6)).save(mixed / "base.jpg", quality=90)
    return plain, mixed


def test_perspcut_views_do_not_change(panos, tmp_path):
    plain, mixed = panos
    for name, src, n in (("plain", plain, 3), ("mixed", mixed, 3)):
        base = CUT + ["-i", str(src), "--count", "4", "--size", "64", "--ext", "png"]
        run(base + ["-o", str(tmp_path / (name + "_host"))], None, "failed=0")
        run(base + ["-o", str(tmp_path / (name + "_dev"))], "device", "failed=0")
        host, dev = files_of(tmp_path / (name + "_host")), files_of(tmp_path / (name + "_dev"))
        assert len(host) == 4 * n and host == dev, name


def test_engine_counts_the_device_decodes(panos, tmp_path, monkeypatch):
    from concurrent.futures import ThreadPoolExecutor
    from gs360 import engine
    plain, mixed = panos
    outs = {}
    for decoder in ("host", "device"):
        monkeypatch.setattr(engine.get_engine(), "device_decoder", decoder == "device")      # (the engine reads GS360_JPEG_DECODER once, when it is made)
        before = engine.get_engine().stats()
        for folder in (plain, mixed):
            src = tmp_path / (decoder + "_src_" + folder.name)      # (its own copies: a resident frame of the other run would be reused)
            shutil.copytree(folder, src)
            out = tmp_path / (decoder + "_" + folder.name)
            out.mkdir()
            args = cut.create_arg_parser().parse_args(["-i", str(src), "--count", "2", "--size", "48", "--ext", "png"])
            for attr in ("size", "hfov", "focal_mm"):
                setattr(args, f"{attr}_explicit", getattr(args, f"{attr}_explicit", False))
            args.input_is_video, args.video_bit_depth = False, 8
            files = [p for p in sorted(src.iterdir()) if p.suffix.lower() in cut.EXTS]
            cut.stop_event.clear()
            jobs = cut.build_view_jobs(args, files, out).jobs
            with ThreadPoolExecutor(max_workers=2) as pool:
                assert list(pool.map(cut.run_one, [cmd for cmd, _s, _d in jobs])) == [(0, "")] * len(jobs)
            outs[(decoder, folder.name)] = files_of(out)
        after = engine.get_engine().stats()
        took = after["device_decoded_frames"] - before["device_decoded_frames"]
        left = after["device_decode_fallbacks"] - before["device_decode_fallbacks"]
        # (a frame evicted and read again would count twice; the cache holds these few frames)
        assert (took, left) == ((4, 1) if decoder == "device" else (0, 0))      # a, b, c, base on the device; prog on the host
    for name in ("plain", "mixed"):
        assert outs[("host", name)] == outs[("device", name)] and len(outs[("host", name)]) == 6


def test_dual_fisheye_pair_views_do_not_change(tmp_path):
    shots = tmp_path / "shots"
    shots.mkdir()
    for lens, seed in (("X", 11), ("Y", 12)):
        Image.fromarray(photo(256, 256, seed)).save(shots / f"frame_0000_{lens}.jpg", quality=92)
    xml = tmp_path / "c.xml"
    xml.write_text(SMALL_XML.replace('"240"', '"256"'))
    got = {}
    for decoder in (None, "device"):
        out = tmp_path / ("out_" + (decoder or "host"))
        stdout = run(DF + ["-i", str(shots), "-x", str(xml), "--interpolation", "linear", "--perspective-size", "64", "--perspective-ext", "png",
                           "--workers", "2", "--save-fisheye-output", "--output-dir", str(tmp_path / ("fish_" + (decoder or "host"))),
                           "--perspective-output-dir", str(out)], decoder, "errors=0")
        got[decoder] = (files_of(out), files_of(tmp_path / ("fish_" + (decoder or "host")), "*"))
        line = "[INFO] JPEG decoder: 2 lens images decoded on the device, 0 on the host"
        assert (line in stdout) == (decoder == "device")
    assert len(got[None][0]) == 10 and len(got[None][1]) == 2 and got[None] == got["device"]      # the views and the undistorted lens images
