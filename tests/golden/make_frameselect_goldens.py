#!/usr/bin/env python3
"""Capture what the reference FrameSelector does with replayed scores: its whole main flow and its selection functions.

Runs only in the build container (needs /root/reference).  The reference module is imported with an empty `cv2` module in
sys.modules (nothing of OpenCV is touched once scoring and flow are replaced), and five of its functions are replaced on the
imported module: score_one_record and _compute_flow_magnitudes (replay seeded values), ensure_ffmpeg_available,
_start_memory_monitor and start_cancel_listener (no-ops).  Its main() then runs on folders of zero-byte image files.  Output is
data only: file names, argv lists, the replayed 9-tuples and flow values, and per step the reference's stdout, the CSV text and
the directory listing.  Two substitutions are made in the stdout, and the comparing test makes the same two: the input directory
becomes <IN>, and the number after `auto=` in the `[INFO] workers:` line (half the CPU count of the machine) becomes <AUTO>.

The replay's conventions (tests/test_frameselect_goldens.py replays them into the drop-in): a record's tuple is looked up by the
base name of its primary file (a step's `order` lists the records' primary files as indices into the case's files); the flow replacement raises flow_mag_arr[i] to flows[i] for every record i and returns
len(records) - 1.

    python tests/golden/make_frameselect_goldens.py     # rewrites frameselect_goldens.json
"""
import contextlib
import io
import json
import os
import pathlib
import re
import shutil
import sys
import tempfile
import types

import numpy as np

sys.dont_write_bytecode = True
REF = pathlib.Path("/root/reference")
HERE = pathlib.Path(__file__).resolve().parent
IN_TOKEN, AUTO_TOKEN = "<IN>", "<AUTO>"
BAD_CSV = b"name,score\nframe_0000.png,0.5\n"      # a CSV without the selected column


def load_reference():
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sys.path.insert(0, str(REF / "cli_tools"))
    import gs360_FrameSelector as ref      # (reference; container-only)
    ref.ensure_ffmpeg_available = lambda: None
    ref._start_memory_monitor = lambda *a, **k: None
    ref.start_cancel_listener = lambda: None
    return ref


# ---- seeded inputs -----------------------------------------------------------------------------------------------------------
def score_set(seed, n, kind, none_every=0):
    """n replayed 9-tuples.  kind "edge": the default backend's shape (no features); "hybrid": the opencv hybrid shape."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    sharp = 0.35 + 0.25 * np.sin(t / 7.0) + 0.2 * rng.random(n)
    bright = np.clip(0.45 + 0.35 * np.sin(t / 23.0 + 1.0) + 0.05 * rng.random(n), 0.02, 1.0)
    out = []
    for i in range(n):
        if none_every and i % none_every == 3:
            out.append([None, 0.0, 0.0, 0.0, 1.0, None, None, None, 1.0])
            continue
        b = round(float(bright[i]), 6)
        w = round(1.0 - 0.5 * (1.0 - min(1.0, b / 0.35)), 6)
        s = round(float(sharp[i]), 6)
        if kind == "edge":
            out.append([s, 0.0, 0.0, b, w, None, None, None, 1.0])
        else:
            lap, ten, fft = round(s * s * 900.0, 4), round(s * 4000.0 + 50.0 * rng.random(), 4), round(20.0 + 30.0 * s * rng.random(), 4)
            mf = round(1.0 - 0.4 * (1.0 - ten / (ten + 5000.0)), 6)
            out.append([round((0.6 * lap + 0.3 * ten + 0.1 * fft) * mf, 6), 0.0, round(0.01 * rng.random(), 6), b, w, lap, ten, fft, mf])
    return out


def flow_set(seed, n):
    """n flow values: calm stretches (runs of low values) and bursts, so that prune and motion augmentation both act."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    base = 1.2 + 1.0 * np.sin(t / 9.0) + 0.3 * rng.random(n)
    base[(t // 12) % 3 == 0] *= 0.05
    base[(t // 15) % 4 == 1] *= 4.0
    return [round(float(v), 5) for v in np.maximum(base, 0.001)]


def frame_names(n, ext=".png"):
    return [f"frame_{i:04d}{ext}" for i in range(n)]


def pair_names(n):
    return [f"shot{i:03d}{lens}.jpg" for i in range(n) for lens in ("_X", "_Y")]


TRICKY = ["B_2.png", "a_10.png", "a_9.PNG", "c1_7.jpg", "C1_07.tif", "b_03.jpeg", "Z.png", "a.tiff", "frame9.png", "frame10.png",
          "Frame11.png", "x_1_2.png", "x_2_1.png", "10.png", "9.png", "skip.txt", "notes.md"]


def tricky_names(n):
    return TRICKY + [f"seq_{(7 * i) % n:03d}_{i % 5}.png" for i in range(n - len(TRICKY) + 2)]


# ---- cases: name -> {files, scores, flows, steps: [{argv (after -i IN), remove (files deleted before the step)}]} --------------------
def cases():
    W = ["-w", "2"]
    out = {}

    def case(name, files, scores, steps, flows=None, mtimes=None):
        out[name] = {"files": files, "scores": scores, "flows": flows, "mtimes": mtimes,
                     "steps": [{"argv": W + s[0], "remove": s[1] if len(s) > 1 else []} for s in steps]}
    # a selection shows in the listing of a real run (kept in place, the rest under blur/); a CSV is written where its columns matter
    case("default_dry_csv", frame_names(64), "edge", [(["-c", "sel.csv", "-d"],)])
    case("default_moves", frame_names(64), "edge", [([],)])
    case("hybrid_all_augmentations", frame_names(96), "hybrid",
         [(["--score_backend", "opencv", "-m", "hybrid", "--augment_motion", "--augment_lowlight", "--prune_motion", "-c", "sel.csv", "-d"],)],
         flows="flow")
    case("lapvar_opencv_moves", frame_names(64), "hybrid", [(["--score_backend", "opencv", "-m", "lapvar", "--no-ignore-highlights", "-n", "8"],)])
    case("gap_mode_strict", frame_names(90), "edge", [(["--augment_gap_mode", "strict", "-n", "12"],)])
    case("no_gaps_no_reopt", frame_names(64), "edge", [(["--no_augment_gaps", "--no-segment-boundary-reopt"],)])
    case("per_frame_n0", frame_names(64), "edge", [(["-n", "0", "--blur-percent", "10", "-c", "sel.csv", "-d"],)])
    case("per_frame_n1", frame_names(64), "edge", [(["-n", "1", "--blur-percent", "2.5", "--augment_lowlight"],)])
    case("min_spacing_zero", frame_names(64), "edge", [(["--min_spacing_frames", "0"],)])
    case("min_spacing_large_lowlight", frame_names(90), "edge", [(["--min_spacing_frames", "6", "--augment_lowlight", "-n", "15"],)])
    case("pair_mode_flow", pair_names(60), "hybrid", [(["-n", "5", "--compute_optical_flow", "-c", "pairs.csv"],)], flows="flow")
    case("pair_mode_forced_unmatched", pair_names(30) + ["stray.jpg", "lonely_X.jpg"], "hybrid", [(["--input_mode", "pair"],)])
    case("auto_mode_incomplete_pairs_are_singles", pair_names(30) + ["lonely_X.jpg"], "edge", [([],)])
    for rule in ("lastnum", "firstnum", "name", "mtime"):
        names = tricky_names(60)
        case(f"sort_{rule}", names, "edge", [(["-s", rule, "-e", "all", "-n", "6"] + (["-c", "sorted.csv", "-d"] if rule == "lastnum" else []),)],
             mtimes=[1700000000 + ((37 * k) % 61) * 10 for k in range(len(names))])
    case("ext_png_only", tricky_names(60), "edge", [(["-e", "png", "-n", "4"],)])
    case("csv_then_reselect_then_apply", frame_names(96), "edge",
         [(["--compute_optical_flow", "-c", "run.csv", "-d"],),
          (["-r", "run.csv", "-n", "6", "--augment_motion", "--prune_motion", "--augment_gap_mode", "strict"],),
          (["-a", "run.csv"], ["frame_0007.png", "frame_0050.png"]),
          (["-a", "run.csv", "--prune_motion"],)], flows="flow")
    case("reselect_without_flow_computes_it", frame_names(64), "edge",
         [(["-c", "run.csv", "-d"],), (["-r", "run.csv", "--prune_motion", "-n", "8"],), (["-a", "run.csv", "--compute_optical_flow"],)],
         flows="flow")
    case("usage_apply_and_reselect", frame_names(60), "edge", [(["-a", "a.csv", "-r", "b.csv"],)])
    case("usage_csv_not_found", frame_names(60), "edge", [(["-a", "missing.csv"],), (["-r", "missing.csv"],)])
    case("usage_no_images", ["readme.txt"], "edge", [([],)])
    case("usage_bad_csv", frame_names(60) + ["bad.csv"], "edge", [(["-a", "bad.csv"],), (["-r", "bad.csv"],)])
    return out


def score_sets():
    return {"edge": score_set(5, 96, "edge", none_every=19), "hybrid": score_set(6, 96, "hybrid", none_every=23)}


def flow_sets():
    return {"flow": flow_set(11, 96)}


# ---- running the reference -----------------------------------------------------------------------------------------------------
def listing(root):
    return sorted(str(p.relative_to(root)).replace(os.sep, "/") + ("/" if p.is_dir() else "") for p in pathlib.Path(root).rglob("*"))


def tokenise(text, in_dir):
    text = text.replace(str(in_dir), IN_TOKEN)
    return re.sub(r"(\[INFO\] workers: .*auto=)\d+", lambda m: m.group(1) + AUTO_TOKEN, text)


def populate(root, case):
    for k, name in enumerate(case["files"]):
        p = pathlib.Path(root) / name
        p.write_bytes(BAD_CSV if name == "bad.csv" else b"")
        if case["mtimes"]:
            os.utime(p, (case["mtimes"][k], case["mtimes"][k]))


def run_case(ref, case, scores, flows):
    """-> the steps' records: stdout, exit (None, an int or the SystemExit message), the CSVs' text and the listing afterwards"""
    root = tempfile.mkdtemp(prefix="fsel_")
    try:
        populate(root, case)
        by_name = {}

        def replay_score(record, *a):
            return tuple(by_name[os.path.basename(record["primary_path"])])

        def replay_flow(records, flow_mag_arr, *a, **k):
            for i in range(len(records)):
                flow_mag_arr[i] = max(flow_mag_arr[i], flows[i])
            return len(records) - 1
        ref.score_one_record, ref._compute_flow_magnitudes = replay_score, replay_flow
        done = []
        for step in case["steps"]:
            for name in step["remove"]:
                os.remove(os.path.join(root, name))
            argv = ["-i", root] + step["argv"]
            # the order the reference itself gives the records decides which replayed tuple a file gets
            files = ref.gather_files(root, argv[argv.index("-e") + 1] if "-e" in argv else "all")
            sorter = ref.SORTERS[argv[argv.index("-s") + 1] if "-s" in argv else "lastnum"]
            try:
                mode = argv[argv.index("--input_mode") + 1] if "--input_mode" in argv else "auto"
                _, recs = ref.build_input_records(files, mode, sorter) if files else (None, [])
            except SystemExit:
                recs = []
            by_name.clear()
            by_name.update({os.path.basename(r["primary_path"]): scores[k] for k, r in enumerate(recs)})
            ref.cancel_event.clear()
            buf, code = io.StringIO(), None
            old_argv = sys.argv
            sys.argv = ["gs360_FrameSelector.py"] + argv
            try:
                with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(io.StringIO()):
                    ref.main()
            except SystemExit as e:
                code = e.code
            finally:
                sys.argv = old_argv
            csvs = {p.name: p.read_text() for p in sorted(pathlib.Path(root).glob("*.csv")) if p.name != "bad.csv"}
            done.append({"argv": step["argv"], "remove": step["remove"], "stdout": tokenise(buf.getvalue(), root), "exit": code,
                         "csv": csvs, "listing": listing(root),
                         "order": [case["files"].index(os.path.basename(r["primary_path"])) for r in recs]})
        return done
    finally:
        shutil.rmtree(root, ignore_errors=True)


def dedupe_csv(steps, store):
    """store each distinct CSV text once: steps refer to it by key"""
    for st in steps:
        for name, text in list(st["csv"].items()):
            key = next((k for k, v in store.items() if v == text), None)
            if key is None:
                key = f"csv{len(store)}"
                store[key] = text
            st["csv"][name] = key


# ---- direct vectors of the selection functions -----------------------------------------------------------------------------------
def function_vectors(ref):
    rng = np.random.default_rng(77)
    vec = {name: [] for name in ("_spacing_respects", "_pick_even_candidate", "_pick_best_between", "augment_spacing",
                                 "evenly_distribute_indices", "augment_motion_segments", "augment_lowlight_segments",
                                 "refine_segment_selection_boundary_local")}

    def scores_of(n, none_rate=0.1):
        return [None if rng.random() < none_rate else round(float(rng.random()), 4) for _ in range(n)]

    def groups(n, size):
        return [{"start": s, "end": min(n, s + size)} for s in range(0, n, size)]
    for _ in range(16):
        sel = sorted(int(v) for v in rng.choice(60, size=int(rng.integers(0, 9)), replace=False))
        cand, md = int(rng.integers(0, 60)), int(rng.integers(0, 8))
        vec["_spacing_respects"].append({"args": [sel, cand, md], "out": ref._spacing_respects(sel, cand, md)})
    for _ in range(6):
        n = int(rng.integers(20, 56))
        missing = set(int(v) for v in rng.choice(n, size=n // 10, replace=False))
        existing = [i for i in range(n) if i not in missing]
        sc = scores_of(n)
        initial = sorted(int(v) for v in rng.choice(existing, size=max(1, len(existing) // 10), replace=False))
        used = sorted(int(v) for v in rng.choice(existing, size=len(existing) // 8, replace=False))
        ordered = sorted(set(used))
        md, fw = int(rng.integers(0, 6)), int(rng.choice([2, 8, 40]))
        target = int(rng.integers(0, len(existing)))
        vec["_pick_even_candidate"].append({"args": [existing, initial, sc, used, target, ordered, md, fw],
                                            "out": ref._pick_even_candidate(existing, set(initial), sc, set(used), target, ordered, md, fw)})
        a, b = sorted(int(v) for v in rng.choice(len(existing), size=2, replace=False))
        tb = (a + b) // 2
        vec["_pick_best_between"].append({"args": [existing, sc, used, a, b, tb, initial, ordered, md, fw],
                                          "out": ref._pick_best_between(existing, sc, set(used), a, b, tb, set(initial), ordered, md, fw)})
        final = sorted(set(initial) | set(int(v) for v in rng.choice(existing, size=3, replace=False)))
        for mode in ("single", "strict"):
            ms = int(rng.integers(0, 14))
            vec["augment_spacing"].append({"args": [final, existing, sc, initial, ms, md, mode, fw],
                                           "out": sorted(ref.augment_spacing(set(final), existing, sc, set(initial), ms, md, mode, fw))})
        vec["evenly_distribute_indices"].append({"args": [existing, initial, sc, md, fw],
                                                 "out": sorted(ref.evenly_distribute_indices(existing, set(initial), sc, md, fw))})
        gi = groups(n, int(rng.integers(4, 16)))
        flow = [round(float(v), 4) for v in rng.gamma(1.5, 1.0, size=n) * (rng.random(n) > 0.2)]
        vec["augment_motion_segments"].append({"args": [final, gi, existing, sc, flow, md],
                                               "out": sorted(ref.augment_motion_segments(set(final), gi, existing, sc, flow, md))})
        bm = [round(float(v), 4) for v in rng.random(n)]
        kr, mk = float(rng.choice([0.0, 0.1, 0.2, 0.5])), int(rng.choice([0, 0, 1, 2]))
        vec["augment_lowlight_segments"].append({"args": [final, gi, existing, sc, bm, md, kr, mk],
                                                 "out": sorted(ref.augment_lowlight_segments(set(final), gi, existing, sc, bm, md, kr, mk))})
    # the boundary re-optimisation reads the records' files: a folder of empty files, some of them missing
    root = tempfile.mkdtemp(prefix="fsel_vec_")
    try:
        for _ in range(6):
            n = int(rng.integers(12, 56))
            missing = sorted(int(v) for v in rng.choice(n, size=n // 12, replace=False))
            for i in range(n):
                p = pathlib.Path(root) / f"f{i:04d}.png"
                if i in missing:
                    p.unlink(missing_ok=True)
                else:
                    p.write_bytes(b"")
            records = [{"file_paths": [str(pathlib.Path(root) / f"f{i:04d}.png")]} for i in range(n)]
            sc = scores_of(n, 0.15)
            gi = groups(n, int(rng.integers(3, 14)))
            initial = set()
            for g in gi:
                ok = [i for i in range(g["start"], g["end"]) if i not in missing and sc[i] is not None]
                if ok:
                    initial.add(max(ok, key=lambda i: (sc[i], -i)))
            md, tk, mp = int(rng.integers(1, 7)), int(rng.integers(1, 5)), int(rng.integers(1, 4))
            out = ref.refine_segment_selection_boundary_local(gi, records, sc, set(initial), md, tk, mp)
            vec["refine_segment_selection_boundary_local"].append({"n": n, "missing": missing, "args": [gi, sc, sorted(initial), md, tk, mp],
                                                                   "out": sorted(out)})
    finally:
        shutil.rmtree(root, ignore_errors=True)
    return vec


def parser_table(ref):
    """dest -> default, flags, choices and type name of every option of the reference's parser (captured while main() builds it)"""
    table = {}
    real = ref.argparse.ArgumentParser.parse_args

    def spy(self, *a, **k):
        for act in self._actions:
            if act.dest == "help":
                continue
            table.setdefault(act.dest, []).append({"flags": list(act.option_strings), "default": act.default,
                                                   "choices": list(act.choices) if act.choices else None,
                                                   "type": getattr(act.type, "__name__", None), "nargs": act.nargs, "const": act.const,
                                                   "required": act.required})
        raise SystemExit(0)
    ref.argparse.ArgumentParser.parse_args = spy
    try:
        ref.main()
    except SystemExit:
        pass
    finally:
        ref.argparse.ArgumentParser.parse_args = real
    return table


def main():
    ref = load_reference()
    sets, flows = score_sets(), flow_sets()
    out = {"source": "cli_tools/gs360_FrameSelector.py main() and its selection functions, on replayed scores (see this generator's docstring)",
           "tokens": {"in_dir": IN_TOKEN, "auto_workers": AUTO_TOKEN}, "parser": parser_table(ref), "score_sets": sets, "flow_sets": flows,
           "csv_texts": {}, "cases": {}}
    for name, case in cases().items():
        steps = run_case(ref, case, sets[case["scores"]], flows[case["flows"]] if case["flows"] else None)
        dedupe_csv(steps, out["csv_texts"])
        out["cases"][name] = {"files": case["files"], "mtimes": case["mtimes"], "scores": case["scores"], "flows": case["flows"], "steps": steps}
    out["functions"] = function_vectors(ref)
    # what the cases must exercise
    text = "\n".join(st["stdout"] + str(st["exit"]) for c in out["cases"].values() for st in c["steps"])
    for pattern in (r"Gap augmentation added [1-9]", r"Low-light augmentation added [1-9]", r"Motion augmentation added [1-9]",
                    r"Motion prune removed [1-9]", r"segment boundary reopt adjusted [1-9]", r"Optical flow computed for [1-9]",
                    r"Optical flow reused from reselect CSV", r" Skipped [1-9]", r"Pair mode requires complete", r"Input mode pair"):
        assert re.search(pattern, text), pattern
    path = HERE / "frameselect_goldens.json"
    path.write_text(json.dumps(out, indent=None, separators=(",", ":")) + "\n")
    print(path, path.stat().st_size, "bytes;", len(out["cases"]), "cases;", sum(len(v) for v in out["functions"].values()), "function vectors")


if __name__ == "__main__":
    main()
