"""VID-COLOR v1 (gs360_video_rgb) on 8K frames: 16 DISTINCT 7680 x 3840 4:2:0 frames per call, at 8 and at 10
bits.  One call reads 16 x 44 (88) MB and writes 16 x 88 (177) MB, several times the 256 MB Infinity Cache, so every call finds its
frames in HBM whatever ran before (HBM-cold by size; nothing is flushed between calls).  HIP events around the call, 3 warm calls, then
the median (with min and max) of `--reps` calls (>= 20); microseconds per frame and bytes moved over time are set against the
memory-system probe's reading on the same GPU right after (lib/libgs360probe.so through bench.memsys_probe).  The NumPy restatement
(tests/vidcolor_np.py) is timed on ONE frame on the same host, and the device's first frame is compared with it.

    python tests/tools/bench_vidcolor.py [--reps 20] [--out profiles/r24/vidcolor/bench_vidcolor.json]      (prints one JSON object)
"""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[2]
for p in (str(ROOT), str(ROOT / "360cam-pgm-3dgs-tools_amd"), str(ROOT / "tests")):
    sys.path.insert(0, p)

import gs360  # noqa: E402
from gs360 import vidcolor  # noqa: E402

import vidcolor_np as ref  # noqa: E402

W, H, N = 7680, 3840, 16


def frames(depth):
    """photo-like planes: smooth fields plus noise, a different phase per frame"""
    rng = np.random.default_rng(depth)
    dt = np.uint8 if depth == 8 else np.uint16
    s = 1 << (depth - 8)
    x = np.arange(W, dtype=np.float32)[None, :]
    y = np.arange(H, dtype=np.float32)[:, None]
    base = 126 + 90 * np.sin(x / 310.0) * np.cos(y / 270.0)
    cbase = 128 + 60 * np.sin(x[:, ::2] / 500.0 + 1.0) * np.cos(y[::2] / 410.0)
    out = []
    for k in range(N):
        Y = np.clip((base + 8 * k + rng.normal(0, 3, base.shape).astype(np.float32)) * s, 16 * s, 235 * s).astype(dt)
        U = np.clip((cbase + 2 * k + rng.normal(0, 2, cbase.shape).astype(np.float32)) * s, 16 * s, 240 * s).astype(dt)
        V = np.clip((256 - cbase - 3 * k) * s, 16 * s, 240 * s).astype(dt)
        out.append((Y, U, V))
    return out


def bench_depth(ctx, depth, reps):
    item = 1 if depth == 8 else 2
    stage = vidcolor.VideoColor(depth)
    host = frames(depth)
    planes = [[ctx.to_device(p) for p in f] for f in host]
    dsts = [ctx.alloc(H * W * 3 * item) for _ in range(N)]
    jobs = [(p[0], p[1], p[2], W, H, "420", d) for p, d in zip(planes, dsts)]

    def call():
        ctx.event_record(0, 0)
        stage.convert_dev(ctx, jobs)
        ctx.event_record(0, 1)
        ctx.sync(0)
        return ctx.event_elapsed_ms(0, 0, 1)
    for _ in range(3):
        call()
    ms = [call() for _ in range(max(20, reps))]
    got = ctx.download(dsts[0], (H, W, 3), dtype=np.uint8 if depth == 8 else np.uint16)
    t0 = time.perf_counter()
    want = ref.convert(*host[0], depth, "420")
    numpy_s = time.perf_counter() - t0
    moved = N * (H * W * item * 1.5 + H * W * 3 * item)
    med = float(np.median(ms))
    for b in [p for f in planes for p in f] + dsts:
        ctx.free(b)
    stage.close()
    return {"depth": depth, "frames_per_call": N, "width": W, "height": H, "subsampling": "420", "reps": len(ms),
            "ms_per_call_median": med, "ms_per_call_min": float(min(ms)), "ms_per_call_max": float(max(ms)),
            "us_per_frame": 1e3 * med / N, "bytes_moved_per_call": moved, "gb_per_s": moved / (med * 1e-3) / 1e9,
            "equals_numpy_restatement": bool(np.array_equal(got, want)), "numpy_restatement_s_per_frame": numpy_s,
            "numpy_over_device": numpy_s / (1e-3 * med / N)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    with gs360.Context(device=0, n_slots=1) as ctx:
        res["device"] = ctx.info()["name"]
        for depth in (8, 10):
            res[f"d{depth}"] = bench_depth(ctx, depth, a.reps)
    import bench
    res["memsys_probe_gb_per_s"] = bench.memsys_probe(0)
    if res["memsys_probe_gb_per_s"]:
        top = max(res["memsys_probe_gb_per_s"].values())
        for depth in (8, 10):
            res[f"d{depth}"]["fraction_of_probe_best"] = res[f"d{depth}"]["gb_per_s"] / top
    print(json.dumps(res, sort_keys=True))
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
