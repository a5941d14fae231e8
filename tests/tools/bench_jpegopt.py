"""Device JPEG encode with the Annex K tables (gs360_jpeg_scan_u8) against per-image optimal tables (gs360_jpeg_scan_opt_u8), same
views, same process: the 12 x 1600^2 views of tests/tools/bench_jpegenc.py's photo-like 8K frame (the full360coverage preset's
geometry), resident, at qualities 100 and 95.

  time    one call over the 12 views, HIP events around it, three warm-up calls, then the two modes ALTERNATED, median of `--reps`
          (30) calls each, per view
  bytes   file bytes per view: device standard, device optimal, Pillow optimize=True and optimize=False, and the ratios
  moved   bytes downloaded per view, each way: lengths + scan (+ 1 088 bytes of tables with optimal tables)
  split   the optimal call with the count pass cut into 64 / 256 / 1024 runs per image and with one wavefront per restart interval

The optimal mode's extra time by pass (count, tables, size + emit) is read from a kernel trace of this program (--trace-reps N runs
only the N alternated calls at quality 100, for a profiler to wrap).

    python tests/tools/bench_jpegopt.py [--reps 30] [--out FILE]     (prints one JSON object)
"""
import argparse
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[2]
for p in (str(ROOT / "360cam-pgm-3dgs-tools_amd"), str(ROOT / "tests"), str(ROOT / "tests" / "tools")):
    sys.path.insert(0, p)

import gs360  # noqa: E402
from gs360 import jpegenc  # noqa: E402

from bench_jpegenc import RESTART, SIZE, pillow_bytes, synth  # noqa: E402

TB = 4 * jpegenc.TABLE_BYTES
COUNT_WAVES = (64, 256, 1024, 8192)


def bench(reps, qualities, trace_only=False):
    views = [gs360.View.make(90.0 * i, 0.0, 104.25, 104.25, SIZE, SIZE) for i in range(4)]
    views += [gs360.View.make(45 + 90.0 * i, p, 104.25, 104.25, SIZE, SIZE) for i in range(4) for p in (30.0, -30.0)]
    n, raw = len(views), SIZE * SIZE * 3
    out = {"views": n, "size": SIZE, "restart_interval": RESTART, "reps": reps, "raw_bytes_per_view": raw, "quality": {}}
    with gs360.Context(device=0, n_slots=1) as ctx:
        d_src = ctx.to_device(synth(3840, 7680))
        d_views = [ctx.alloc(raw) for _ in views]
        ctx.equirect_views_dev([d_src], 7680, 3840, 3, views, d_views)
        ctx.sync(0)
        arrays = [ctx.download(d, (SIZE, SIZE, 3)) for d in d_views]
        d_out = [ctx.alloc(raw) for _ in views]
        d_len, d_tab = ctx.alloc(8 * n), ctx.alloc(TB * n)
        jobs = [(d, SIZE, SIZE, 3, 0, o, raw) for d, o in zip(d_views, d_out)]
        out["device"] = ctx.info()["name"]

        def encode(optimal, quality):
            ctx.event_record(0, 0)
            if optimal:
                ctx.jpeg_scan_opt_dev(jobs, d_len, d_tab, quality=quality, restart=RESTART)
            else:
                ctx.jpeg_scan_dev(jobs, d_len, quality=quality, restart=RESTART)
            ctx.event_record(0, 1)
            return ctx.event_elapsed_ms(0, 0, 1)

        for quality in qualities:
            for _ in range(3):
                encode(False, quality)
                encode(True, quality)
            ms = {False: [], True: []}
            for _ in range(reps):
                for optimal in (False, True):
                    ms[optimal].append(encode(optimal, quality))
            if trace_only:
                continue
            encode(False, quality)
            len_std = [int(v) for v in ctx.download(d_len, (n,), np.uint64)]
            encode(True, quality)
            len_opt = [int(v) for v in ctx.download(d_len, (n,), np.uint64)]
            tabs = ctx.download(d_tab, (n, TB), np.uint8)
            assert max(len_std + len_opt) <= raw, "a scan did not fit the view's raw size"
            head_std = len(jpegenc.header(SIZE, SIZE, 3, quality, RESTART)) + 2
            head_opt = [len(jpegenc.header(SIZE, SIZE, 3, quality, RESTART, t.tobytes())) + 2 for t in tabs]
            r = {"standard_ms_per_view": float(np.median(ms[False])) / n, "optimal_ms_per_view": float(np.median(ms[True])) / n,
                 "standard_ms_per_call_min_max": [float(min(ms[False])), float(max(ms[False]))],
                 "optimal_ms_per_call_min_max": [float(min(ms[True])), float(max(ms[True]))],
                 "standard_file_bytes_per_view": float(np.mean(len_std)) + head_std,
                 "optimal_file_bytes_per_view": float(np.mean(len_opt)) + float(np.mean(head_opt)),
                 "standard_downloaded_bytes_per_view": float(np.mean(len_std)) + 8,
                 "optimal_downloaded_bytes_per_view": float(np.mean(len_opt)) + 8 + TB,
                 "pillow_optimize_file_bytes_per_view": float(np.mean([pillow_bytes(a, quality, True) for a in arrays])),
                 "pillow_plain_file_bytes_per_view": float(np.mean([pillow_bytes(a, quality, False) for a in arrays]))}
            # the count pass's split (context option jpeg_count_waves; 8192 is above the 5000 intervals of a view: one flush per interval)
            sweep = {w: [] for w in COUNT_WAVES}
            for w in COUNT_WAVES:
                with ctx.options(jpeg_count_waves=w):
                    encode(True, quality)
            for _ in range(reps):
                for w in COUNT_WAVES:
                    with ctx.options(jpeg_count_waves=w):
                        sweep[w].append(encode(True, quality))
            r["optimal_ms_per_call_by_count_waves"] = {str(w): float(np.median(v)) for w, v in sweep.items()}
            r["optimal_ms_over_standard_ms"] = r["optimal_ms_per_view"] / r["standard_ms_per_view"]
            r["optimal_bytes_over_standard"] = r["optimal_file_bytes_per_view"] / r["standard_file_bytes_per_view"]
            r["optimal_bytes_over_pillow_optimize"] = r["optimal_file_bytes_per_view"] / r["pillow_optimize_file_bytes_per_view"]
            r["standard_bytes_over_pillow_plain"] = r["standard_file_bytes_per_view"] / r["pillow_plain_file_bytes_per_view"]
            out["quality"][str(quality)] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--trace-reps", type=int, default=0, help="only N alternated calls at quality 100 (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.trace_reps:
        bench(a.trace_reps, [100], trace_only=True)
        return
    res = bench(a.reps, [100, 95])
    print(json.dumps(res, sort_keys=True))
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
