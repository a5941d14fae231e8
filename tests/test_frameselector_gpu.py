"""The FrameSelector drop-in end to end on the MI355X, as the GUI runs it (a subprocess with an argv): the CSV's score, brightness
and flow columns against the NumPy restatements of the three passes, its selected column against gs360.frameselect on those
columns, then the moves of a real run."""
import csv
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import frameedge_np as enp
import frameflow_np as ffn
import framescore_np as fnp
from gs360 import frameselect as fsel
from gs360 import framescore, imageio

pytestmark = pytest.mark.gpu

CLI = pathlib.Path(__file__).resolve().parents[1] / "360cam-pgm-3dgs-tools_amd" / "cli_tools" / "gs360_FrameSelector.py"


def _sequence(seed, n, H, W):
    """n frames of a drifting blocky texture, each blurred by 0-4 passes of a 3-tap mean and dimmed a little: graded sharpness"""
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


def _run(argv):
    """a fresh child process, as the GUI starts the tool; its stdout"""
    done = subprocess.run([sys.executable, str(CLI)] + argv, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert done.returncode == 0, done.stdout
    return done.stdout


def _rows(path):
    with open(path, newline="") as f:
        return list(csv.DictReader(f))


def _expected_selection(scores, brightness_mean, records, segment_size):
    """gs360.frameselect on the CSV's own columns, with the default flags' steps (grouping, boundary re-optimisation, gap filling)"""
    plan = fsel.spacing_plan(segment_size, None, False, False)
    existing = list(range(len(scores)))
    groups = fsel.group_segments(scores, [1.0] * len(scores), brightness_mean, segment_size, [0.0] * len(scores))
    initial = fsel.initial_picks(groups, scores, existing)
    initial = fsel.refine_segment_selection_boundary_local(groups, records, scores, initial, plan["min_diff"]) & set(existing)
    return fsel.augment_spacing(initial, existing, scores, initial, plan["max_spacing"], plan["min_diff"], "single", plan["fast_window"])


def _flow_column(values, n):
    """a record's flow_motion: the larger of the values of the pairs it belongs to"""
    col = [0.0] * n
    for k, v in enumerate(values):
        v = 9999.0 if v is None else v
        col[k], col[k + 1] = max(col[k], v), max(col[k + 1], v)
    return col


@pytest.fixture(scope="module")
def singles(tmp_path_factory):
    root = tmp_path_factory.mktemp("frames")
    frames = _sequence(60, 60, 120, 200)
    for i, f in enumerate(frames):
        imageio.write_image(root / f"frame_{i:04d}.png", f)
    return root, frames


def test_default_backend_csv_then_a_real_run(singles):
    root, frames = singles
    n = len(frames)
    out = _run(["-i", str(root), "-c", "sel.csv", "-d"])
    assert "[INFO] score_backend=ffmpeg uses sobel+signalstats; --metric ignored." in out and f" Input records {n}" in out
    rows = _rows(root / "sel.csv")
    assert [r["filename"] for r in rows] == [f"frame_{i:04d}.png" for i in range(n)]
    want = [enp.score(f, 0.8) for f in frames]
    assert [float(r["score"]) for r in rows] == [w[0] for w in want]                    # exact: integer sums, %g, one division
    assert [float(r["brightness_mean"]) for r in rows] == [w[3] for w in want]
    assert len({w[0] for w in want}) > n // 2                                             # graded, not constant
    records = [{"file_paths": [str(root / r["filename"])]} for r in rows]
    keep = _expected_selection([float(r["score"]) for r in rows], [float(r["brightness_mean"]) for r in rows], records, 10)
    assert {i for i, r in enumerate(rows) if r["selected(1=keep)"] == "1"} == keep and 0 < len(keep) < n
    assert sorted(os.listdir(root / "blur")) == []                                        # the dry run moved nothing
    # the real run
    out = _run(["-i", str(root)])
    assert f" Kept {len(keep)}\n Moved {n - len(keep)} \n Skipped 0\n" in out
    assert {p for p in os.listdir(root) if p.endswith(".png")} == {f"frame_{i:04d}.png" for i in keep}
    assert set(os.listdir(root / "blur")) == {f"frame_{i:04d}.png" for i in range(n)} - {f"frame_{i:04d}.png" for i in keep}


def test_opencv_hybrid_with_flow_csv(tmp_path):
    frames = _sequence(61, 60, 120, 200)
    n = len(frames)
    for i, f in enumerate(frames):
        imageio.write_image(tmp_path / f"frame_{i:04d}.png", f)
    out = _run(["-i", str(tmp_path), "--score_backend", "opencv", "-m", "hybrid", "--compute_optical_flow", "-c", "sel.csv", "-d"])
    assert f"Optical flow computed for {n - 1} pair(s):" in out
    rows = _rows(tmp_path / "sel.csv")
    tuples = [fnp.score(f, "hybrid", 0.8, False, True) for f in frames]
    want = framescore.hybrid_scores(tuples)
    # the fft feature carries the float32 INTER_AREA image (1e-5 relative, as tests/test_framescore_gpu.py); it enters the score
    # normalised over the run's range and weighted 0.1, so 1e-5 absolute covers it with room
    assert [float(r["score"]) for r in rows] == pytest.approx(want, rel=1e-5, abs=1e-5)
    assert [float(r["brightness_mean"]) for r in rows] == [t[3] for t in tuples]
    flows = ffn.flow_values(frames, [(k, k + 1) for k in range(n - 1)], fsel.FLOW_CROP_RATIO, "none")
    assert [float(r["flow_motion"]) for r in rows] == _flow_column(flows, n)           # exact, as tests/test_frameflow_gpu.py
    assert any(0.0 < v < 9999.0 for v in _flow_column(flows, n))
    records = [{"file_paths": [str(tmp_path / r["filename"])]} for r in rows]
    keep = _expected_selection([float(r["score"]) for r in rows], [float(r["brightness_mean"]) for r in rows], records, 10)
    assert {i for i, r in enumerate(rows) if r["selected(1=keep)"] == "1"} == keep


def test_pair_folder(tmp_path):
    xs, ys = _sequence(62, 20, 160, 160), _sequence(63, 20, 160, 160)
    n = len(xs)
    for i, (x, y) in enumerate(zip(xs, ys)):
        imageio.write_image(tmp_path / f"shot{i:03d}_X.png", x)
        imageio.write_image(tmp_path / f"shot{i:03d}_Y.png", y)
    out = _run(["-i", str(tmp_path), "-n", "5", "--compute_optical_flow", "-c", "pairs.csv", "-d"])
    assert "[INFO] pair mode uses a circular fisheye mask; switching score backend ffmpeg -> opencv" in out
    assert " Input mode pair\n" in out and f" Source files {2 * n}\n" in out
    rows = _rows(tmp_path / "pairs.csv")
    assert [(r["filename"], r["x_filename"], r["y_filename"]) for r in rows] == \
        [(f"shot{i:03d}", f"shot{i:03d}_X.png", f"shot{i:03d}_Y.png") for i in range(n)]
    tuples = [framescore.average_tuples([fnp.score(a, "hybrid", 1.0, False, True, "fisheye_circle") for a in (x, y)]) for x, y in zip(xs, ys)]
    assert [float(r["score"]) for r in rows] == pytest.approx(framescore.hybrid_scores(tuples), rel=1e-5, abs=1e-5)
    assert [float(r["brightness_mean"]) for r in rows] == [t[3] for t in tuples]
    pairs = [(k, k + 1) for k in range(n - 1)]
    fx, fy = ffn.flow_values(xs, pairs, 1.0, "fisheye_circle"), ffn.flow_values(ys, pairs, 1.0, "fisheye_circle")
    values = [framescore.mean_finite([a, b]) for a, b in zip(fx, fy)]
    assert [float(r["flow_motion"]) for r in rows] == _flow_column(values, n)
    records = [{"file_paths": [str(tmp_path / r["x_filename"]), str(tmp_path / r["y_filename"])]} for r in rows]
    keep = _expected_selection([float(r["score"]) for r in rows], [float(r["brightness_mean"]) for r in rows], records, 5)
    assert {i for i, r in enumerate(rows) if r["selected(1=keep)"] == "1"} == keep


def test_sixteen_bit_source_is_one_error_line_and_nothing_moves(tmp_path):
    frames = _sequence(64, 12, 60, 80)
    for i, f in enumerate(frames):
        imageio.write_image(tmp_path / f"f{i:02d}.png", f)
    imageio.write_image(tmp_path / "f05.png", frames[5].astype(np.uint16) * 257)
    done = subprocess.run([sys.executable, str(CLI), "-i", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert done.returncode == 1
    assert [line for line in done.stdout.replace("\r", "\n").splitlines() if line.startswith("[ERR]")] != []
    assert len([p for p in os.listdir(tmp_path) if p.endswith(".png")]) == 12 and os.listdir(tmp_path / "blur") == []
