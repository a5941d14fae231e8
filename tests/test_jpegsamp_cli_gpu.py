"""-m gpu: GS360_JPEG_DECODER=device through the two drop-in tools on 4:2:2, 4:4:0 and 4:1:1 inputs.  The views are written as PNG,
so the comparison is of pixels: a run with the device decoder writes byte for byte the files of the host decoder's run, and the
engine's counters show that all three layouts were decoded on the device and none fell back to the host."""
import shutil
import sys

import pytest

pytest.importorskip("PIL.Image")
from PIL import Image  # noqa: E402

import gs360_360PerspCut as cut  # noqa: E402
from conftest import PKG  # noqa: E402
from test_dualfisheye_cli import SMALL_XML  # noqa: E402
from test_jpegdec_cli_gpu import files_of, photo, run  # noqa: E402

import jpegsamp_np as samp  # noqa: E402

pytestmark = pytest.mark.gpu
CUT = [sys.executable, str(PKG / "cli_tools" / "gs360_360PerspCut.py")]
DF = [sys.executable, str(PKG / "cli_tools" / "gs360_DualFisheyeDistortionCalibration.py")]


@pytest.fixture(scope="module")
def panos(tmp_path_factory):
    folder = tmp_path_factory.mktemp("jps_cut") / "panos"
    folder.mkdir()
    Image.fromarray(photo(256, 512, 1)).save(folder / "a422.jpg", quality=92, subsampling=1)
    (folder / "b440.jpg").write_bytes(samp.write(photo(256, 512, 2), 1, 2, 90, 0))
    (folder / "c411.jpeg").write_bytes(samp.write(photo(256, 512, 3), 4, 1, 85, 16))
    return folder


def test_perspcut_views_do_not_change(panos, tmp_path):
    base = CUT + ["-i", str(panos), "--count", "4", "--size", "64", "--ext", "png"]
    run(base + ["-o", str(tmp_path / "host")], None, "failed=0")
    run(base + ["-o", str(tmp_path / "dev")], "device", "failed=0")
    host, dev = files_of(tmp_path / "host"), files_of(tmp_path / "dev")
    assert len(host) == 4 * 3 and host == dev


def test_engine_counts_the_device_decodes(panos, tmp_path, monkeypatch):
    from concurrent.futures import ThreadPoolExecutor
    from gs360 import engine
    outs = {}
    for decoder in ("host", "device"):
        monkeypatch.setattr(engine.get_engine(), "device_decoder", decoder == "device")      # (the engine reads GS360_JPEG_DECODER once, when it is made)
        before = engine.get_engine().stats()
        src = tmp_path / (decoder + "_src")      # (its own copies: a resident frame of the other run would be reused)
        shutil.copytree(panos, src)
        out = tmp_path / decoder
        out.mkdir()
        args = cut.create_arg_parser().parse_args(["-i", str(src), "--count", "2", "--size", "48", "--ext", "png"])
        for attr in ("size", "hfov", "focal_mm"):
            setattr(args, f"{attr}_explicit", getattr(args, f"{attr}_explicit", False))
        args.input_is_video, args.video_bit_depth = False, 8
        files = [p for p in sorted(src.iterdir()) if p.suffix.lower() in cut.EXTS]
        assert len(files) == 3
        cut.stop_event.clear()
        jobs = cut.build_view_jobs(args, files, out).jobs
        with ThreadPoolExecutor(max_workers=2) as pool:
            assert list(pool.map(cut.run_one, [cmd for cmd, _s, _d in jobs])) == [(0, "")] * len(jobs)
        outs[decoder] = files_of(out)
        after = engine.get_engine().stats()
        took = after["device_decoded_frames"] - before["device_decoded_frames"]
        left = after["device_decode_fallbacks"] - before["device_decode_fallbacks"]
        assert (took, left) == ((3, 0) if decoder == "device" else (0, 0))
    assert outs["host"] == outs["device"] and len(outs["host"]) == 6


def test_dual_fisheye_pair_views_do_not_change(tmp_path):
    shots = tmp_path / "shots"
    shots.mkdir()
    for lens, seed in (("X", 11), ("Y", 12)):
        Image.fromarray(photo(256, 256, seed)).save(shots / f"frame_0000_{lens}.jpg", quality=92, subsampling=1)
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
