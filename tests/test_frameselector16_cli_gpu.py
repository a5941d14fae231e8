"""The FrameSelector drop-in on 16-bit frames (FS-DEPTH16 v1), as the GUI runs it: a child process with GS360_FS_DEPTH16=device in
its environment only.  The 12-frame folder of tests/test_frameselector_gpu.py's 16-bit test, every frame a gray PNG: written as
16-bit `* 257` it must give the CSV of the same folder written as 8-bit (statistics pass: the sums are the 8-bit sums times the
unit; edge and flow pass: the 8-bit view of 257 v is v)."""
import csv
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import framescore_np as fnp
from gs360 import imageio
from test_frameselector_gpu import _sequence

pytestmark = pytest.mark.gpu

CLI = pathlib.Path(__file__).resolve().parents[1] / "360cam-pgm-3dgs-tools_amd" / "cli_tools" / "gs360_FrameSelector.py"
COUNT_LINE = "[INFO] 16-bit frames: {} scored and tracked at full depth on the device"


def _child(argv, depth16):
    env = {k: v for k, v in os.environ.items() if k != "GS360_FS_DEPTH16"}
    if depth16 is not None:
        env["GS360_FS_DEPTH16"] = depth16
    return subprocess.run([sys.executable, str(CLI)] + argv, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300,
                          env=env)


def _rows(path):
    with open(path, newline="") as f:
        return list(csv.DictReader(f))


def _lines(done, prefix):
    return [line for line in done.stdout.replace("\r", "\n").splitlines() if line.startswith(prefix)]


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    """(8-bit folder, 16-bit folder, mixed folder) of the same 12 gray frames."""
    grays = [fnp.gray_u8(f).astype(np.uint8) for f in _sequence(64, 12, 60, 80)]
    roots = [tmp_path_factory.mktemp(name) for name in ("gray8", "gray16", "mixed")]
    for i, g in enumerate(grays):
        g16 = g.astype(np.uint16) * 257
        imageio.write_image(roots[0] / f"f{i:02d}.png", g)
        imageio.write_image(roots[1] / f"f{i:02d}.png", g16)
        imageio.write_image(roots[2] / f"f{i:02d}.png", g16 if i % 2 else g)
    assert imageio.read_image(roots[1] / "f03.png").dtype == np.uint16
    return roots


COLUMNS = ("filename", "score", "brightness_mean", "flow_motion", "selected(1=keep)")


def _csv_of(root, argv, depth16):
    done = _child(["-i", str(root), "-c", "sel.csv", "-d", "-n", "4", "--compute_optical_flow"] + argv, depth16)
    assert done.returncode == 0, done.stdout
    rows = _rows(root / "sel.csv")
    assert len(rows) == 12 and os.listdir(root / "blur") == []
    return done, [tuple(r[c] for c in COLUMNS) for r in rows]


_eight_bit_runs = {}              # argv -> the 8-bit folder's run, shared by the tests that compare against it


def _eight_bit(folders, argv):
    if tuple(argv) not in _eight_bit_runs:
        _eight_bit_runs[tuple(argv)] = _csv_of(folders[0], argv, None)
    return _eight_bit_runs[tuple(argv)]


# ignore_highlights is the CLI's default: the opencv runs take the highlight mask (243 <-> 62451 >= 62259, 242 <-> 62194 < 62259)
@pytest.mark.parametrize("argv", [["--score_backend", "opencv", "-m", "hybrid"],
                                  ["--score_backend", "opencv", "-m", "lapvar", "--no-ignore-highlights", "--fft", "device"],
                                  ["--score_backend", "opencv", "-m", "fft", "--fft", "device"],
                                  []], ids=["opencv-hybrid-host-fft", "opencv-lapvar", "opencv-device-fft", "default-backend"])
def test_sixteen_bit_folder_gives_the_csv_of_its_eight_bit_folder(folders, argv):
    done8, want = _eight_bit(folders, argv)
    done16, got = _csv_of(folders[1], argv, "device")
    assert _lines(done16, "[INFO] 16-bit frames") == [COUNT_LINE.format(12)] and _lines(done8, "[INFO] 16-bit frames") == []
    assert got == want                                              # the CSV's text: scores, brightness, flow, selection
    assert len({g[1] for g in got}) > 6 and any(0.0 < float(g[3]) < 9999.0 for g in got)
    assert 0 < sum(g[4] == "1" for g in got) < 12


def test_pair_folder(tmp_path):
    """Pair mode (the circle mask in the statistics and the flow pass): 8 X / Y pairs, as 16-bit `* 257` and as 8-bit."""
    xs = [fnp.gray_u8(f).astype(np.uint8) for f in _sequence(62, 8, 96, 96)]
    ys = [fnp.gray_u8(f).astype(np.uint8) for f in _sequence(63, 8, 96, 96)]
    csvs = []
    for name, scale, depth16 in (("p8", None, None), ("p16", 257, "device")):
        root = tmp_path / name
        root.mkdir()
        for i, (x, y) in enumerate(zip(xs, ys)):
            for tag, g in (("X", x), ("Y", y)):
                imageio.write_image(root / f"shot{i:03d}_{tag}.png", g if scale is None else g.astype(np.uint16) * scale)
        done = _child(["-i", str(root), "-n", "4", "--compute_optical_flow", "-c", "pairs.csv", "-d"], depth16)
        assert done.returncode == 0, done.stdout
        assert " Input mode pair\n" in done.stdout
        assert _lines(done, "[INFO] 16-bit frames") == ([COUNT_LINE.format(16)] if depth16 else [])
        csvs.append([tuple(r[c] for c in COLUMNS) for r in _rows(root / "pairs.csv")])
    assert csvs[1] == csvs[0] and len(csvs[0]) == 8
    assert len({c[1] for c in csvs[0]}) > 4 and any(0.0 < float(c[3]) < 9999.0 for c in csvs[0])


def test_mixed_folder_runs_and_moves(folders):
    root = folders[2]
    _, want = _eight_bit(folders, [])
    done = _child(["-i", str(root), "-n", "4", "--compute_optical_flow"], "device")
    assert done.returncode == 0, done.stdout
    assert _lines(done, "[INFO] 16-bit frames") == [COUNT_LINE.format(6)] and _lines(done, "[ERR]") == []
    keep = {w[0] for w in want if w[4] == "1"}
    assert {p for p in os.listdir(root) if p.endswith(".png")} == keep
    assert set(os.listdir(root / "blur")) == {w[0] for w in want} - keep


def test_switch_off_or_wrong_is_one_error_line_and_nothing_moves(folders):
    root = folders[1]
    for value, text in ((None, "8-bit"), ("off", "8-bit"), ("host", "GS360_FS_DEPTH16")):
        done = _child(["-i", str(root)], value)
        errs = _lines(done, "[ERR]")
        assert done.returncode == 1 and len(errs) == 1 and text in errs[0], done.stdout
        assert len([p for p in os.listdir(root) if p.endswith(".png")]) == 12
        assert not (root / "blur").exists() or os.listdir(root / "blur") == []
