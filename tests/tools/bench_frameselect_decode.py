"""The FrameSelector's reader with the device JPEG decoder (GS360_JPEG_DECODER=device, gs360/framesource.py) against the host decoder,
on 7680 x 3840 4:2:0 quality-92 JPEG frames (tests/tools/bench_jpegdec.py's photo-like frames), same box, same run.

  kernels  16 distinct files per call.  One gs360_jpeg_decode_u8 call (RGB frames) and one gs360_jpeg_decode_gray_u8 call (gray
           planes) per repetition, in turn, then gs360_frame_stats_u8 (fs_strip_kernel, the lapvar statistics with the highlight mask)
           on the 16 RGB frames (C = 3) and on the 16 gray planes (C = 1), in turn.  One call's coefficients, frames and planes are
           some gigabytes, far beyond the 256 MiB Infinity Cache, so every kernel reads its inputs from HBM.  Device-event times per
           call are printed; the kernel times come from running this mode under the profiler, with nothing else traced:
               rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python tests/tools/bench_frameselect_decode.py kernels
           and reading jd_pixels_kernel<false> / <true> and fs_strip_kernel<3, false> / <1, false> from NAME_kernel_stats.csv
           (AverageNs per call of 16 frames).
  cli      `gs360_FrameSelector.py -c sel.csv -d --compute_optical_flow` on a folder of --frames (64) such files, as fresh child
           processes with GS360_JPEG_DECODER=host and =device in turn, --runs (3) each: wall time of the whole process, the
           device run's [INFO] counts (decoded, fallbacks, reused), and whether the CSV files are byte-identical.  The host run is the
           parent commit's path.

One process per mode, a time limit on every child process, no retries: a step that fails ends the tool with its output.

    python tests/tools/bench_frameselect_decode.py kernels [--reps 10] [--frames 16] [--width 7680] [--out FILE]
    python tests/tools/bench_frameselect_decode.py cli [--frames 64] [--runs 3] [--width 7680] [--dir DIR] [--out FILE]
    (each prints one JSON object)
"""
import argparse
import concurrent.futures
import io
import json
import os
import pathlib
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[2]
for p in (str(ROOT / "360cam-pgm-3dgs-tools_amd"), str(ROOT / "tests"), str(ROOT / "tests" / "tools")):
    sys.path.insert(0, p)

CLI = ROOT / "360cam-pgm-3dgs-tools_amd" / "cli_tools" / "gs360_FrameSelector.py"
INFO = re.compile(r"\[INFO\] JPEG decoder: (\d+) frames decoded on the device, (\d+) fallbacks, (\d+) reused")
CHILD_TIMEOUT_S = 600


def files(frames, width):
    """-> [file bytes] of `frames` distinct frames, encoded on a few threads (Pillow releases the GIL)"""
    from PIL import Image
    from bench_jpegdec import synth
    base = synth(width // 2, width)

    def one(k):
        b = io.BytesIO()
        Image.fromarray(np.roll(base, (37 * k, 131 * k), axis=(0, 1))).save(b, "JPEG", quality=92, subsampling=2)
        return b.getvalue()
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
        return list(ex.map(one, range(frames)))


def _timed(ctx, call):
    ctx.event_record(0, 0)
    call()
    ctx.event_record(0, 1)
    ctx.sync(0)
    return ctx.event_elapsed_ms(0, 0, 1)


def kernels(reps, frames, width):
    import gs360
    from gs360 import capi, framescore, jpegdec
    height = width // 2
    datas = files(frames, width)
    out = {"frames": frames, "width": width, "height": height, "reps": reps, "file_bytes_per_frame": int(np.mean([len(d) for d in datas]))}
    with gs360.Context(device=0, n_slots=1) as ctx:
        prepared = [jpegdec.prepare(d) for d in datas]
        t0 = time.perf_counter()
        rgb = jpegdec.Batch(ctx, prepared)
        gray = jpegdec.Batch(ctx, prepared, gray=True)
        out["alloc_upload_ms_per_frame"] = (time.perf_counter() - t0) * 1e3 / (2 * frames)
        stats = ctx.alloc(frames * capi.C.sizeof(capi.FrameStats))
        try:
            for b in (rgb, gray):
                b.run()
                assert b.status() == [0] * frames
            ms = {"decode_rgb": [], "decode_gray": [], "stats_c3": [], "stats_c1": []}
            for _ in range(reps):
                ms["decode_rgb"].append(_timed(ctx, rgb.run))
                ms["decode_gray"].append(_timed(ctx, gray.run))
            band = framescore.band_rows(height, 0.8)
            planes = {3: [it[2] for it in rgb.items], 1: [it[2] for it in gray.items]}
            recs = {}
            for _ in range(reps + 1):
                for c in (3, 1):
                    t = _timed(ctx, lambda: ctx.frame_stats_dev(planes[c], height, width, c, band, stats, flags=capi.FS_HIGHLIGHTS))
                    ms["stats_c%d" % c].append(t)
                    recs[c] = ctx.download(stats, (frames, len(framescore.FIELDS)), np.int64)
            out["statistics_equal"] = bool(np.array_equal(recs[3], recs[1]))
            for k, v in ms.items():
                v = v[1:] if k.startswith("stats") else v                      # (the first statistics launch loads the code object)
                out[k + "_ms_per_frame"] = statistics.median(v) / frames
                out[k + "_ms_per_call_min_max"] = [min(v), max(v)]
        finally:
            ctx.free(stats)
            rgb.close()
            gray.close()
    return out


def cli(frames, runs, width, folder):
    root = pathlib.Path(folder) if folder else pathlib.Path(tempfile.mkdtemp(prefix="fsdec_"))
    root.mkdir(parents=True, exist_ok=True)
    sizes = []
    for k, data in enumerate(files(frames, width)):
        (root / f"frame_{k:04d}.jpg").write_bytes(data)
        sizes.append(len(data))
    out = {"frames": frames, "width": width, "height": width // 2, "runs": runs, "file_bytes_per_frame": int(np.mean(sizes)),
           "argv": "-c <csv> -d --compute_optical_flow", "wall_s": {"host": [], "device": []}, "device_counts": []}
    for r in range(runs):
        for mode in ("host", "device"):
            env = dict(os.environ, GS360_JPEG_DECODER=mode)
            t0 = time.perf_counter()
            done = subprocess.run([sys.executable, str(CLI), "-i", str(root), "-c", f"{mode}.csv", "-d", "--compute_optical_flow"],
                                  stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=CHILD_TIMEOUT_S)
            wall = time.perf_counter() - t0
            if done.returncode != 0:
                raise SystemExit(f"{mode} run {r} ended with {done.returncode}:\n{done.stdout[-3000:]}")
            out["wall_s"][mode].append(wall)
            m = INFO.search(done.stdout)
            if mode == "device":
                out["device_counts"].append(dict(zip(("device_decoded", "fallbacks", "reused"), map(int, m.groups()))) if m else None)
        out.setdefault("csv_identical", []).append((root / "host.csv").read_bytes() == (root / "device.csv").read_bytes())
    for mode in ("host", "device"):
        out[f"wall_s_median_{mode}"] = statistics.median(out["wall_s"][mode])
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernels", "cli"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--width", type=int, default=7680)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = kernels(a.reps, a.frames or 16, a.width) if a.mode == "kernels" else cli(a.frames or 64, a.runs, a.width, a.dir)
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")
