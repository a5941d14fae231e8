"""Device JPEG encode with 2 x 2 chroma subsampling (gs360_jpeg_scan_sub_u8, GS360_JPEG_420: the dual-fisheye tool's files) against
the 4:4:4 call (GS360_JPEG_444: the code of gs360_jpeg_scan_u8 / gs360_jpeg_scan_opt_u8), same views, same process: ten resident
1750^2 RGB views (the tool's SFM10 default) cut from tests/tools/bench_jpegenc.py's photo-like 8K frame, at qualities 95 and 100,
with the Annex K tables and with optimal tables.

  time     one call over the 10 views, HIP events around it, three warm-up calls, then the four modes ALTERNATED, median of `--reps`
           (30) calls each, per call and per view
  restart  the 4:2:0 standard call at restart intervals of 4 and 8 MCUs (16 x 16 pixels each), alternated the same way
  bytes    file bytes per view: device 4:2:0 standard and optimal, device 4:4:4, Pillow subsampling=2 with optimize False and True
  moved    bytes downloaded per view: lengths + scan (+ 1 088 bytes of tables with optimal tables), against the raw view

Where a 4:2:0 call is slower than its 4:4:4 twin, the pass is read from a kernel trace of this program (--trace-reps N runs only the
N alternated calls at quality 100, for a profiler to wrap).

    python tests/tools/bench_jpeg420.py [--reps 30] [--out FILE]     (prints one JSON object)
"""
import argparse
import io
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[2]
for p in (str(ROOT / "360cam-pgm-3dgs-tools_amd"), str(ROOT / "tests"), str(ROOT / "tests" / "tools")):
    sys.path.insert(0, p)

import gs360  # noqa: E402
from gs360 import capi, jpegenc  # noqa: E402

from bench_jpegenc import RESTART, synth  # noqa: E402

SIZE = 1750
TB = 4 * jpegenc.TABLE_BYTES
MODES = [("444_standard", capi.JPEG_444, False), ("420_standard", capi.JPEG_420, False),
         ("444_optimal", capi.JPEG_444, True), ("420_optimal", capi.JPEG_420, True)]
NAME = {capi.JPEG_444: "4:4:4", capi.JPEG_420: "4:2:0"}


def pillow_bytes(a, quality, optimize):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", quality=quality, subsampling=2, optimize=optimize)
    return b.tell()


def bench(reps, qualities, trace_only=False):
    views = [gs360.View.make(90.0 * i, 0.0, 104.25, 104.25, SIZE, SIZE) for i in range(4)]
    views += [gs360.View.make(45 + 90.0 * i, p, 104.25, 104.25, SIZE, SIZE) for i in range(3) for p in (30.0, -30.0)]
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

        def encode(sub, optimal, quality, restart=RESTART):
            ctx.event_record(0, 0)
            ctx.jpeg_scan_sub_dev(jobs, d_len, d_tab if optimal else None, quality=quality, restart=restart, subsampling=sub)
            ctx.event_record(0, 1)
            return ctx.event_elapsed_ms(0, 0, 1)

        for quality in qualities:
            for _ in range(3):
                for _name, sub, optimal in MODES:
                    encode(sub, optimal, quality)
            ms = {name: [] for name, _s, _o in MODES}
            for _ in range(reps):
                for name, sub, optimal in MODES:
                    ms[name].append(encode(sub, optimal, quality))
            if trace_only:
                continue
            r = {}
            for name, sub, optimal in MODES:
                encode(sub, optimal, quality)
                lengths = [int(v) for v in ctx.download(d_len, (n,), np.uint64)]
                assert max(lengths) <= raw, "a scan did not fit the view's raw size"
                tabs = ctx.download(d_tab, (n, TB), np.uint8) if optimal else [None] * n
                heads = [len(jpegenc.header(SIZE, SIZE, 3, quality, RESTART, None if t is None else t.tobytes(), NAME[sub])) + 2 for t in tabs]
                r[name] = {"ms_per_call": float(np.median(ms[name])), "ms_per_view": float(np.median(ms[name])) / n,
                           "ms_per_call_min_max": [float(min(ms[name])), float(max(ms[name]))],
                           "file_bytes_per_view": float(np.mean(lengths)) + float(np.mean(heads)),
                           "downloaded_bytes_per_view": float(np.mean(lengths)) + 8 + (TB if optimal else 0)}
            # the restart interval: 16 x 16 MCUs make an interval of 8 a wavefront's walk of 48 blocks (24 in 4:4:4)
            sweep = {4: [], 8: []}
            for ri in sweep:
                encode(capi.JPEG_420, False, quality, ri)
            for _ in range(reps):
                for ri in sweep:
                    sweep[ri].append(encode(capi.JPEG_420, False, quality, ri))
            r["420_standard_ms_per_call_by_restart_interval"] = {str(ri): float(np.median(v)) for ri, v in sweep.items()}
            r["pillow_420_plain_file_bytes_per_view"] = float(np.mean([pillow_bytes(a, quality, False) for a in arrays]))
            r["pillow_420_optimize_file_bytes_per_view"] = float(np.mean([pillow_bytes(a, quality, True) for a in arrays]))
            r["420_over_444_ms_standard"] = r["420_standard"]["ms_per_call"] / r["444_standard"]["ms_per_call"]
            r["420_over_444_ms_optimal"] = r["420_optimal"]["ms_per_call"] / r["444_optimal"]["ms_per_call"]
            r["420_over_444_bytes_standard"] = r["420_standard"]["file_bytes_per_view"] / r["444_standard"]["file_bytes_per_view"]
            r["420_standard_bytes_over_pillow_plain"] = r["420_standard"]["file_bytes_per_view"] / r["pillow_420_plain_file_bytes_per_view"]
            r["420_optimal_bytes_over_pillow_optimize"] = r["420_optimal"]["file_bytes_per_view"] / r["pillow_420_optimize_file_bytes_per_view"]
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
    res = bench(a.reps, [95, 100])
    print(json.dumps(res, sort_keys=True))
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
