"""The FrameSelector drop-in's command line: every reference flag with the reference's destination, default, choices and type
behaviour (the golden stores them from the reference's own parser), the usage errors with their exit codes, and --dry_run.
No GPU: where a run scores, the scores are replayed through main()'s seam keywords."""
import argparse
import contextlib
import io
import json
import os

import pytest

import gs360_FrameSelector as cli

from conftest import GOLDEN

G = json.loads((GOLDEN / "frameselect_goldens.json").read_text())
OWN_FLAGS = {"fft"}                     # additive options of this build

# what each of the reference's type functions takes and refuses (FS:271-309)
TYPE_SAMPLES = {
    "segment_size_arg": (["0", "1", "10"], ["-1", "x", "1.5"]),
    "non_negative_int": (["0", "3"], ["-1", "x"]),
    "ratio_in_0_1": (["1", "0.8", "1e-3"], ["0", "1.01", "-0.5", "x", "nan"]),
    "percent_0_100": (["0", "2.5", "100"], ["-1", "100.5", "x", "nan"]),
    "int": (["2", "-3"], ["x", "1.5"]),
}


def _actions():
    return {a.dest: a for a in cli.build_parser()._actions if a.dest != "help"}


def test_every_reference_option_with_its_destination_default_choices_and_type():
    ours = {}
    for act in cli.build_parser()._actions:
        if act.dest != "help":
            ours.setdefault(act.dest, []).append(act)
    assert set(ours) - OWN_FLAGS == set(G["parser"])
    for dest, entries in G["parser"].items():
        assert len(entries) == len(ours[dest]), dest
        for want, act in zip(entries, ours[dest]):
            assert list(act.option_strings) == want["flags"], dest
            assert act.default == want["default"], dest
            assert (list(act.choices) if act.choices else None) == want["choices"], dest
            assert (act.nargs, act.const, act.required) == (want["nargs"], want["const"], want["required"]), dest
            assert (act.type is None) == (want["type"] is None), dest
            if want["type"]:
                good, bad = TYPE_SAMPLES[want["type"]]
                for text in good:
                    assert act.type(text) == (int(text) if want["type"] in ("int", "segment_size_arg", "non_negative_int") else float(text))
                for text in bad:
                    with pytest.raises((argparse.ArgumentTypeError, ValueError)):
                        act.type(text)


def test_defaults_namespace():
    args = cli.build_parser().parse_args(["-i", "frames"])
    want = {dest: entries[0]["default"] for dest, entries in G["parser"].items()}
    want["in_dir"] = "frames"
    got = vars(args)
    assert {k: got[k] for k in want} == want and got["fft"] is None


def test_gui_style_argv_parses():
    """every flag the GUI composes for the tool (reference gs360_GUI.py:10270-10447), in its spelling"""
    argv = ["-i", "/data/frames", "-n", "12", "--dry_run", "-c", "sel.csv", "-m", "lapvar", "--score_backend", "opencv", "-e", "jpg", "-s", "name",
            "--input_mode", "single", "-w", "8", "--score_crop_ratio", "0.7", "--min_spacing_frames", "3", "--augment_gaps", "--no_augment_gaps",
            "--augment_gap_mode", "strict", "--augment_lowlight", "--compute_optical_flow", "--augment_motion",
            "--no-segment-boundary-reopt", "--blur-percent", "5", "--prune_motion", "--no-ignore-highlights"]
    a = cli.build_parser().parse_args(argv)
    assert (a.segment_size, a.dry_run, a.csv, a.metric, a.score_backend, a.ext, a.sort, a.input_mode, a.workers) == \
        (12, True, "sel.csv", "lapvar", "opencv", "jpg", "name", "single", 8)
    assert (a.score_crop_ratio, a.min_spacing_frames, a.augment_gaps, a.augment_gap_mode, a.augment_lowlight, a.compute_optical_flow,
            a.augment_motion, a.segment_boundary_reopt, a.blur_percent, a.prune_motion, a.ignore_highlights) == \
        (0.7, 3, False, "strict", True, True, True, False, 5.0, True, False)


@pytest.mark.parametrize("argv", [[], ["-i", "x", "-n", "-1"], ["-i", "x", "--score_crop_ratio", "0"], ["-i", "x", "--blur-percent", "101"],
                                  ["-i", "x", "-m", "sobel"], ["-i", "x", "--fft", "gpu"], ["-i", "x", "--min_spacing_frames", "-2"]])
def test_argparse_usage_errors_exit_2(argv):
    with pytest.raises(SystemExit) as e, contextlib.redirect_stderr(io.StringIO()):
        cli.main(argv)
    assert e.value.code == 2


def _run(argv, **kw):
    out, code = io.StringIO(), None
    cli.cancel_event.clear()
    try:
        with contextlib.redirect_stdout(out):
            cli.main(argv, **kw)
    except SystemExit as e:
        code = e.code
    return code, out.getvalue()


def _frames(root, n=30):
    for i in range(n):
        (root / f"f{i:03d}.png").write_bytes(b"")
    return sorted(os.listdir(root))


def _replay(records, *a, **kw):
    return [(0.1 + (7 * k % 10) / 20.0, 0.0, 0.0, 0.5, 1.0, None, None, None, 1.0) for k in range(len(records))]


def test_exit_messages_and_codes(tmp_path):
    empty = tmp_path / "empty"
    empty.mkdir()
    assert _run(["-i", str(empty)]) == (1, f"No input images found: {empty}\n")
    frames = tmp_path / "frames"
    frames.mkdir()
    _frames(frames)
    assert _run(["-i", str(frames), "-a", "a.csv", "-r", "b.csv"])[0] == "--apply_csv and --reselect_csv cannot be used together."
    code, out = _run(["-i", str(frames), "-a", "nope.csv"])
    assert code == 1 and out.endswith(f"Selection CSV not found: {frames / 'nope.csv'}\n")
    code, out = _run(["-i", str(frames), "-r", str(tmp_path / "abs.csv")])
    assert code == 1 and out.endswith(f"Metrics CSV not found: {tmp_path / 'abs.csv'}\n")
    (frames / "bad.csv").write_text("index,score\n0,0.5\n")
    code, out = _run(["-i", str(frames), "-a", "bad.csv"])
    assert code == 1 and out.endswith("Failed to load selection CSV: CSV missing 'selected(1=keep)' column\n")
    code, out = _run(["-i", str(frames), "-r", "bad.csv"])
    assert code == 1 and out.endswith("Failed to load metrics CSV: CSV missing 'selected(1=keep)' column\n")
    (frames / "lonely_X.png").write_bytes(b"")
    assert _run(["-i", str(frames), "--input_mode", "pair"])[0] == \
        "Pair mode requires complete _X/_Y image pairs only. unmatched_files=30, incomplete_pairs=1"
    pairless = tmp_path / "pairless"
    pairless.mkdir()
    (pairless / "only.txt.png").write_bytes(b"")
    assert _run(["-i", str(pairless), "--input_mode", "pair"])[0].startswith("Pair mode requires complete")


def test_unsupported_source_ends_the_run_before_any_move(tmp_path):
    from gs360 import capi
    names = _frames(tmp_path)

    def sixteen_bit(records, *a, **kw):
        raise capi.Gs360Error(-4, "frame scoring takes 8-bit images (got uint16); 16-bit and float sources are not implemented")
    code, out = _run(["-i", str(tmp_path)], score_records=sixteen_bit)
    assert code == 1 and out.splitlines()[-1].startswith("[ERR] ") and "8-bit" in out.splitlines()[-1]
    assert sorted(os.listdir(tmp_path)) == sorted(names + ["blur"]) and os.listdir(tmp_path / "blur") == []


def test_dry_run_moves_nothing_and_a_run_moves_the_rest(tmp_path):
    names = _frames(tmp_path)
    code, out = _run(["-i", str(tmp_path), "-d", "-c", "sel.csv", "-w", "1"], score_records=_replay)
    assert code is None and "Blur directory (dry run, no files moved):" in out
    assert sorted(os.listdir(tmp_path)) == sorted(names + ["blur", "sel.csv"]) and os.listdir(tmp_path / "blur") == []
    rows = (tmp_path / "sel.csv").read_text().splitlines()
    assert rows[0] == "index,input_mode,filename,pair_base,x_filename,y_filename,score,brightness_mean,group_score,flow_motion,selected(1=keep)"
    keep = {r.split(",")[2] for r in rows[1:] if r.endswith(",1")}
    assert 0 < len(keep) < len(names)
    code, out = _run(["-i", str(tmp_path), "-a", "sel.csv"])
    assert code is None and f" Kept {len(keep)}\n Moved {len(names) - len(keep)} \n" in out
    assert {n for n in os.listdir(tmp_path) if n.endswith(".png")} == keep
    assert set(os.listdir(tmp_path / "blur")) == set(names) - keep


def test_cancelled_run_says_so_and_moves_nothing(tmp_path):
    names = _frames(tmp_path)

    def cancel_midway(records, *a, progress=None, **kw):
        cli.cancel_event.set()
        progress(1)
    code, out = _run(["-i", str(tmp_path)], score_records=cancel_midway)
    cli.cancel_event.clear()
    assert code is None and "Cancelled by user. Partial results may be incomplete." in out
    assert {n for n in os.listdir(tmp_path) if n.endswith(".png")} == set(names)
