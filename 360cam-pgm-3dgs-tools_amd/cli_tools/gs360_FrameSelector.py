#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""gs360_FrameSelector -- MI355X drop-in for the reference tool of the same name.

The GUI starts this tool as a subprocess with an argv, so the contract is the command line: the reference's flags, destinations,
defaults and type functions (reference cli_tools/gs360_FrameSelector.py:1917-2083), its exit messages and codes, its stdout
lines in its order ([INFO] / [WARN] lines, the Scoring / Optical flow / Grouping progress, the augmentation and flow summaries,
the `Done:` block), its CSV and its moves into <in_dir>/blur.

What changed underneath: every per-pixel pass runs on the GPU through libgs360hip.so.  `--score_backend ffmpeg` (the default)
spawns no ffmpeg: it is the edge pass gs360_frame_edge_u8 (FS-EDGE v1); `--score_backend opencv` is
gs360_frame_stats_u8 (+ gs360_frame_fft_energy with `--fft device`); the optical flow is gs360_frame_flow_u8.  Frames are decoded
on a thread pool (`--workers`, default: gs360.framescore's own, at most 16) that runs ahead of launches of 16 frames; with
GS360_JPEG_DECODER=device baseline .jpg / .jpeg frames are decoded on the GPU instead, once for the scoring and the flow pass
(gs360/framesource.py), and one more [INFO] line counts them.  The
selection itself is gs360/frameselect.py.  8-bit sources by default: a 16-bit or float image ends the run with one [ERR] line and
exit code 1 before anything is moved.  With GS360_FS_DEPTH16=device (FS-DEPTH16 v1) 16-bit PNG / TIFF frames, those Video2Frames
writes for sources of more than 8 bits per sample, are scored (gs360_frame_stats_u16 / gs360_frame_edge_u16), tracked
(gs360_frame_flow_u16), selected and moved like any others, alone or mixed with 8-bit frames, and one more [INFO] line counts them;
any other value of the variable is one [ERR] line.  The reference's memory-pressure limiter and its stdin listener are left out.

main(argv, score_records=..., flow_magnitudes=...) replaces the two GPU seams, for tests that replay recorded scores.
"""
import argparse
import contextlib
import csv
import math
import os
import pathlib
import signal
import sys

_HERE = pathlib.Path(__file__).resolve().parent
if str(_HERE.parent) not in sys.path:
    sys.path.insert(0, str(_HERE.parent))

from gs360 import frameflow, framescore, framesource, jpegdec  # noqa: E402
from gs360 import frameselect as fsel  # noqa: E402
from gs360.capi import Gs360Error  # noqa: E402

cancel_event = frameflow.cancel_event     # one flag for this flow and the flow pass (the reference's module-level event)


def segment_size_arg(value):
    try:
        number = int(value)
    except (TypeError, ValueError):
        number = -1
    if number < 0:
        raise argparse.ArgumentTypeError("--segment_size must be an integer >= 0")
    return number


def non_negative_int(value):
    try:
        number = int(value)
    except (TypeError, ValueError):
        number = -1
    if number < 0:
        raise argparse.ArgumentTypeError("value must be >= 0")
    return number


def _bounded_float(lo_open, lo, hi, message):
    def parse(value):
        try:
            number = float(value)
        except (TypeError, ValueError):
            number = math.nan
        if not ((lo < number if lo_open else lo <= number) and number <= hi):
            raise argparse.ArgumentTypeError(message)
        return number
    return parse


ratio_in_0_1 = _bounded_float(True, 0.0, 1.0, "value must be a float in (0, 1]")
percent_0_100 = _bounded_float(False, 0.0, 100.0, "value must be a percentage in [0, 100]")

# (flags, keywords): names, destinations, types, choices and defaults are the reference's command line (FS:1917-2083); the help
# wording is ours.  The last entry is this build's own.
_OPTIONS = (
    (("-i", "--in_dir"), dict(required=True, help="folder with the frames (not searched recursively)")),
    (("-n", "--segment_size"), dict(type=segment_size_arg, default=10, help="frames per segment; one frame of each is kept (default 10).  "
                                                                           "0 or 1: per-frame mode, see --blur-percent")),
    (("-d", "--dry_run"), dict(action="store_true", help="score and select, move nothing")),
    (("-c", "--csv"), dict(help="write the selection as CSV (absolute, or relative to the input folder)")),
    (("-r", "--reselect_csv"), dict(help="select again from the scores of a CSV written with --csv, without scoring")),
    (("-a", "--apply_csv"), dict(help="move files as a CSV from a dry run says")),
    (("-m", "--metric"), dict(choices=["hybrid", "lapvar", "tenengrad", "fft"], default="hybrid",
                              help="sharpness metric of the opencv backend (default hybrid)")),
    (("--score_backend",), dict(choices=["ffmpeg", "opencv"], default=fsel.DEFAULT_SCORE_BACKEND,
                                help="ffmpeg (default): mean Sobel magnitude, ignores --metric; opencv: --metric")),
    (("-e", "--ext"), dict(choices=["all", "tif", "jpg", "png"], default="all", help="extensions to take (default all)")),
    (("-s", "--sort"), dict(choices=["lastnum", "firstnum", "name", "mtime"], default="lastnum", help="order of the frames")),
    (("--input_mode",), dict(choices=["auto", "single", "pair"], default="auto", help="single images, or _X / _Y fisheye pairs")),
    (("-w", "--workers"), dict(type=int, help="decode threads (default: chosen by the scoring pass, at most 16)")),
    (("--score_crop_ratio",), dict(type=ratio_in_0_1, default=fsel.DEFAULT_CROP_RATIO,
                                   help=f"central band of rows that is scored, (0, 1] (default {fsel.DEFAULT_CROP_RATIO:.1f})")),
    (("--min_spacing_frames",), dict(type=non_negative_int, default=None,
                                     help="frames to keep between selected frames "
                                          f"(default round(segment_size * {fsel.MIN_DIFF_FRAMES_RATIO:.1f}))")),
    (("--augment_gaps",), dict(dest="augment_gaps", action="store_true", default=True, help="fill wide gaps after the selection (default)")),
    (("--no_augment_gaps",), dict(dest="augment_gaps", action="store_false", help="do not fill gaps")),
    (("--augment_gap_mode",), dict(choices=["single", "strict"], default="single",
                                   help="single: one frame per wide gap; strict: until no gap is wider than the limit")),
    (("--augment_lowlight",), dict(action="store_true", help="add frames per segment by brightness-weighted sharpness")),
    (("--compute_optical_flow",), dict(action="store_true", help="fill the flow_motion column; the selection does not use it")),
    (("--augment_motion",), dict(action="store_true", help="add frames in segments with much motion")),
    (("--segment-boundary-reopt",), dict(dest="segment_boundary_reopt", action="store_true", default=True,
                                         help="re-choose neighbouring segments' picks among their sharpest frames (default)")),
    (("--no-segment-boundary-reopt",), dict(dest="segment_boundary_reopt", action="store_false", help="keep each segment's sharpest frame")),
    (("--blur-percent",), dict(type=percent_0_100, default=1.0, help="per-frame mode: percentage of lowest scores to move (default 1.0)")),
    (("--prune_motion",), dict(action="store_true", help="drop selected frames inside runs of very low motion")),
    (("--ignore-highlights",), dict(dest="ignore_highlights", action="store_true", default=True,
                                    help="opencv backend: leave pixels above 95%% brightness out (default)")),
    (("--no-ignore-highlights",), dict(dest="ignore_highlights", action="store_false", help="count clipped highlights")),
    (("--fft",), dict(choices=["host", "device"], default=None, help="where the fft / hybrid metrics' FFT runs (default host)")),
)


def build_parser():
    ap = argparse.ArgumentParser(description="Keep the sharpest frames of a folder; the others go to <in_dir>/blur.")
    for flags, kw in _OPTIONS:
        ap.add_argument(*flags, **kw)
    return ap


def _handle_sigint(signum, frame):
    if not cancel_event.is_set():
        print("\\nCancellation requested (Ctrl+C). Finishing current tasks...")      # (the reference prints the two characters \\n)
        cancel_event.set()


class _Cancelled(Exception):
    pass


_progress = frameflow.update_progress


def _resolve(in_dir, path):
    return path if os.path.isabs(path) else os.path.join(in_dir, path)


def _load_csv(kind, path, records, scores, brightness_mean_arr, group_score_arr, flow_mag_arr):
    """The flags of a CSV given on the command line; kind = "Selection" / "Metrics" words the reference's two failure messages."""
    if not os.path.isfile(path):
        print(f"{kind} CSV not found: {path}")
        sys.exit(1)
    try:
        return fsel.load_selection_from_csv(path, records, scores, brightness_mean_arr, group_score_arr, flow_mag_arr)
    except ValueError as exc:
        print(f"Failed to load {kind.lower()} CSV: {exc}")
        sys.exit(1)


def main(argv=None, *, score_records=None, flow_magnitudes=None):
    args = build_parser().parse_args(argv)
    score_records = score_records or framescore.score_records
    flow_magnitudes = flow_magnitudes or frameflow._compute_flow_magnitudes
    if args.apply_csv and args.reselect_csv:
        raise SystemExit("--apply_csv and --reselect_csv cannot be used together.")
    if args.reselect_csv:
        args.dry_run = True
    scoring_needed = not args.apply_csv and not args.reselect_csv
    try:
        device_decoder = jpegdec.device_decoder_enabled()      # GS360_JPEG_DECODER
        depth16 = framescore.depth16_mode_from_env()           # GS360_FS_DEPTH16
        framescore.depth16_files.clear()
    except ValueError as exc:
        print(f"[ERR] {exc}")
        sys.exit(1)
    cancel = cancel_event
    try:
        signal.signal(signal.SIGINT, _handle_sigint)
    except (ValueError, AttributeError):
        pass

    flow_crop_ratio = fsel.FLOW_CROP_RATIO
    score_crop_ratio = args.score_crop_ratio
    if not (0.0 < score_crop_ratio <= 1.0):
        raise SystemExit("--score_crop_ratio must be in (0, 1]")
    raw_files = fsel.gather_files(args.in_dir, args.ext)
    if not raw_files:
        print(f"No input images found: {args.in_dir}")
        sys.exit(1)
    plan = fsel.spacing_plan(args.segment_size, args.min_spacing_frames, args.augment_motion, bool(args.apply_csv))
    min_diff = plan["min_diff"]

    input_mode, records = fsel.build_input_records(raw_files, args.input_mode, fsel.SORTERS[args.sort])
    if input_mode == "pair":
        if args.score_backend == "ffmpeg":
            print("[INFO] pair mode uses a circular fisheye mask; switching score backend ffmpeg -> opencv")
            args.score_backend = "opencv"
        if not math.isclose(score_crop_ratio, 1.0):
            print(f"[INFO] pair mode uses a circular center mask; overriding --score_crop_ratio {score_crop_ratio:.3f} -> 1.0")
        score_crop_ratio = 1.0
        if not math.isclose(flow_crop_ratio, 1.0):
            print(f"[INFO] pair mode uses a circular center mask for motion; overriding FLOW_CROP_RATIO {flow_crop_ratio:.3f} -> 1.0")
        flow_crop_ratio = 1.0
    if args.score_backend == "ffmpeg" and scoring_needed:
        if args.ignore_highlights:
            print("[INFO] ffmpeg backend ignores --ignore-highlights; disabling.")
            args.ignore_highlights = False
        print("[INFO] score_backend=ffmpeg uses sobel+signalstats; --metric ignored.")

    blur_dir = os.path.join(args.in_dir, "blur")
    os.makedirs(blur_dir, exist_ok=True)

    n = total = len(records)
    exists = fsel.record_exists
    scores = [None] * n
    tuples = None                         # the run's 9-tuples, when it scored
    brightness_arr = [1.0] * n
    brightness_mean_arr = [0.0] * n
    group_score_arr = [0.0] * n
    flow_mag_arr = [0.0] * n
    compute_optical_flow = bool(args.compute_optical_flow or args.prune_motion or args.augment_motion)
    source_file_total = sum(len(r.get("file_paths", [])) for r in records)
    selection_flags = [0] * n
    final_selected, initial_selected = set(), set()
    group_infos, existing_indices = [], []
    added = {"gap": 0, "lowlight": 0, "motion": 0}
    apply_csv_path = reselect_csv_path = None
    reused_flow = False

    # the pool size printed is the reference's (half the CPUs the machine shows); the passes size their own pools unless -w is given
    auto_workers = max(1, (os.cpu_count() or 4) // 2)
    manual = bool(args.workers and args.workers > 0)
    if manual and args.workers > max(1, auto_workers * 2):
        print("[WARN] workers={} exceeds {} (auto={}); continuing.".format(args.workers, max(1, auto_workers * 2), auto_workers))
    workers = args.workers if manual else auto_workers
    pool = args.workers if manual else None
    print("[INFO] workers: {} (mode={}, auto={})".format(workers, "manual" if manual else "auto", auto_workers))

    # GS360_JPEG_DECODER=device: the gray planes decoded for scoring stay in device memory for the flow pass (gs360/framesource.py)
    with framesource.open_store() if device_decoder else contextlib.nullcontext():
        if args.apply_csv:
            apply_csv_path = _resolve(args.in_dir, args.apply_csv)
            selection_flags = _load_csv("Selection", apply_csv_path, records, scores, brightness_mean_arr, group_score_arr, flow_mag_arr)
            final_selected = {i for i, flag in enumerate(selection_flags) if flag == 1 and exists(records[i])}
            initial_selected = set(final_selected)
            existing_indices = [i for i in range(total) if exists(records[i])]
        elif args.reselect_csv:
            reselect_csv_path = _resolve(args.in_dir, args.reselect_csv)
            selection_flags = _load_csv("Metrics", reselect_csv_path, records, scores, brightness_mean_arr, group_score_arr, flow_mag_arr)
            existing_indices = [i for i in range(total) if exists(records[i])]
            if compute_optical_flow:
                reused_flow = fsel.csv_has_numeric_flow_motion_values(reselect_csv_path)
                if reused_flow:
                    print("[INFO] reselect CSV already contains numeric flow_motion values; reusing them without recomputation.")
        else:
            state = {"done": 0, "pct": -1}

            def tick(count):
                if cancel.is_set():
                    raise _Cancelled()
                while state["done"] < min(count, n):
                    state["done"] += 1
                    state["pct"] = _progress("Scoring", state["done"], n, state["pct"])
            try:
                tuples = score_records(records, args.metric, score_crop_ratio, fsel.MAX_LONG, args.augment_motion, args.ignore_highlights,
                                       args.score_backend, workers=pool, fft=args.fft, progress=tick)
                tick(n)
            except (_Cancelled, KeyboardInterrupt):
                cancel.set()
                tuples = None
            except Gs360Error as exc:
                print(f"[ERR] {exc}")
                sys.exit(1)
            if tuples is not None:
                scores = [t[0] for t in tuples]
                brightness_mean_arr = [t[3] for t in tuples]
                brightness_arr = [t[4] for t in tuples]
        cancelled = cancel.is_set()

        flow_pairs_total = 0
        if not cancelled and n > 1 and compute_optical_flow and not reused_flow:
            flow_pairs_total = flow_magnitudes(records, flow_mag_arr, flow_crop_ratio, pool, "Optical flow")
            cancelled = cancel.is_set()
    if device_decoder:
        st = framesource.stats()
        print("[INFO] JPEG decoder: {} frames decoded on the device, {} fallbacks, {} reused".format(
            st["device_decoded"], st["fallbacks"], st["reused"]))
    if depth16:
        print("[INFO] 16-bit frames: {} scored and tracked at full depth on the device".format(len(framescore.depth16_files)))

    if not cancelled and args.metric == "hybrid" and tuples is not None:
        scores = framescore.hybrid_scores(tuples)

    csv_path = None
    if args.csv:
        csv_path = _resolve(args.in_dir, args.csv)
    elif apply_csv_path and compute_optical_flow:
        csv_path = apply_csv_path
    elif reselect_csv_path:
        csv_path = reselect_csv_path
    fcsv = open(csv_path, "w", newline="") if csv_path else None
    writer = csv.writer(fcsv) if fcsv else None
    if writer:
        writer.writerow(fsel.CSV_HEADER)

    if not args.apply_csv and not cancelled:
        existing_indices = [i for i in range(total) if exists(records[i])]
        if args.segment_size <= 1:
            final_selected = fsel.select_per_frame(scores, existing_indices, args.blur_percent)
            initial_selected = set(final_selected)
            args.augment_gaps = args.augment_lowlight = args.augment_motion = False
        else:
            group_infos = fsel.group_segments(scores, brightness_arr, brightness_mean_arr, args.segment_size, group_score_arr)
            initial_selected = fsel.initial_picks(group_infos, scores, existing_indices)
            if args.segment_boundary_reopt and len(group_infos) >= 2:
                before = set(initial_selected)
                initial_selected = fsel.refine_segment_selection_boundary_local(group_infos, records, scores, initial_selected, min_diff)
                initial_selected &= set(existing_indices)
                if initial_selected != before:
                    print("[INFO] segment boundary reopt adjusted {} selection slot(s).".format(len(initial_selected ^ before)))
            final_selected = set(initial_selected)

    if args.prune_motion and not cancelled and final_selected:
        pruned, threshold = fsel.prune_low_motion(final_selected, flow_mag_arr)
        if pruned:
            if args.apply_csv:
                for i in pruned:
                    selection_flags[i] = 0
                final_selected = {i for i in range(n) if selection_flags[i] and exists(records[i])}
                initial_selected = set(final_selected)
            else:
                initial_selected -= pruned
                final_selected -= pruned
                existing_indices = [i for i in existing_indices if i not in pruned]
                initial_selected &= set(existing_indices)
            print(f"Motion prune removed {len(pruned)} frame(s) below P{fsel.FLOW_LOW_MOTION_PERCENTILE:.0f} (threshold {threshold:.4f}).")

    if not args.apply_csv and not cancelled:
        steps = (("gap", args.augment_gaps, lambda sel: fsel.augment_spacing(
                     sel, existing_indices, scores, initial_selected, plan["max_spacing"], min_diff, args.augment_gap_mode, plan["fast_window"])),
                 ("lowlight", args.augment_lowlight, lambda sel: fsel.augment_lowlight_segments(
                     sel, group_infos, existing_indices, scores, brightness_mean_arr, min_diff, fsel.BRIGHTNESS_SHARPNESS_KEEP_RATIO,
                     fsel.BRIGHTNESS_SHARPNESS_MIN_KEEP)),
                 ("motion", args.augment_motion, lambda sel: fsel.augment_motion_segments(
                     sel, group_infos, existing_indices, scores, flow_mag_arr, plan["motion_min_diff"])))
        for name, wanted, step in steps:
            if wanted:
                grown = step(final_selected)
                added[name] = len(grown - final_selected)
                final_selected = grown

    kept = moved = skipped = processed = 0
    last_pct = -1
    for i in range(total):
        if cancel.is_set():
            cancelled = True
            break
        record = records[i]
        s = 0.0 if args.apply_csv and scores[i] is None else scores[i]
        processed += 1
        row = [i, record.get("input_mode", input_mode), *fsel.record_csv_labels(record)]
        if not exists(record) or s is None:
            skipped += 1
            row += [-1.0, 0.0, group_score_arr[i], flow_mag_arr[i], 0]
        else:
            keep = i in final_selected
            if keep:
                kept += 1
            elif args.dry_run:
                moved += 1
            else:
                failures = sum(1 for src in record.get("file_paths", [])
                               if fsel.safe_move(src, os.path.join(blur_dir, os.path.basename(src))) is None)
                skipped += failures
                moved += 0 if failures else 1
            row += [s, brightness_mean_arr[i], group_score_arr[i], flow_mag_arr[i], 1 if keep else 0]
        if writer:
            writer.writerow(row)
        last_pct = _progress("Grouping", processed, total, last_pct)
    cancelled = cancelled or cancel.is_set()
    if fcsv:
        fcsv.close()

    if cancelled:
        print("Cancelled by user. Partial results may be incomplete.")
    for name, wanted, text in (("gap", args.augment_gaps, "Gap"), ("lowlight", args.augment_lowlight, "Low-light"),
                               ("motion", args.augment_motion, "Motion")):
        if wanted:
            print(f"{text} augmentation added {added[name]} frame(s).")
    if compute_optical_flow:
        summary = fsel.flow_summary(flow_mag_arr)
        if summary:
            head = "Optical flow reused from reselect CSV:" if reused_flow else f"Optical flow computed for {flow_pairs_total} pair(s):"
            print("{} min={:.4f}, median={:.4f}, max={:.4f}".format(head, *summary))
        elif n > 1:
            print("Optical flow requested, but no finite pair magnitudes were available.")
    print("Done:")
    print(f" Input records {total}")
    print(f" Input mode {input_mode}")
    print(f" Source files {source_file_total}")
    print(f" Kept {kept}")
    print(f" Moved {moved} ")
    print(f" Skipped {skipped}")
    print("Blur directory (dry run, no files moved):" if args.dry_run else "Blur directory:", blur_dir)
    print(f"workers={workers},  score_crop_ratio={score_crop_ratio}, flow_crop_ratio={flow_crop_ratio}, "
          f"max_spacing={plan['max_spacing']}, min_spacing_frames={plan['base_spacing_frames']}")


if __name__ == "__main__":
    main()
