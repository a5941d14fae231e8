"""VID-FEED v1's (10, 8) instantiation of gs360_video_rgb next to the two of VID-COLOR v1, on 8K frames: 16 DISTINCT 7680 x 3840 4:2:0
frames per call.  One call reads 16 x 44 (88) MB and writes 16 x 88 (177) MB, several times the 256 MB Infinity Cache, so every call
finds its frames in HBM whatever ran before (HBM-cold by size; nothing is flushed between calls).  The three instantiations (8, 8),
(10, 16) and (10, 8) alternate in one process: after 3 warm calls each, `--rounds` rounds of one window per instantiation, a window
being `--calls` calls between one pair of HIP events.  Reported per instantiation: device-event microseconds per frame (median, min
and max over the windows) and the bytes a frame moves, counted from the shapes.  The first frame of (10, 8) is compared with the NumPy
restatement (tests/vidfeed_np.py).

    python tests/tools/bench_vidfeed.py [--rounds 20] [--calls 50] [--out profiles/r28/vidfeed/bench_vidfeed.json]   (prints one JSON object)
"""
import argparse
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[2]
for p in (str(ROOT), str(ROOT / "360cam-pgm-3dgs-tools_amd"), str(ROOT / "tests")):
    sys.path.insert(0, p)

import gs360  # noqa: E402
from gs360 import vidcolor  # noqa: E402

import vidfeed_np as feed_ref  # noqa: E402

W, H, N = 7680, 3840, 16
PAIRS = ((8, 8), (10, 16), (10, 8))


def frames8():
    """photo-like 8-bit planes: smooth fields plus noise, a different phase per frame"""
    rng = np.random.default_rng(28)
    x = np.arange(W, dtype=np.float32)[None, :]
    y = np.arange(H, dtype=np.float32)[:, None]
    base = (126 + 90 * np.sin(x / 310.0) * np.cos(y / 270.0)).astype(np.int16)
    cbase = (128 + 60 * np.sin(x[:, ::2] / 500.0 + 1.0) * np.cos(y[::2] / 410.0)).astype(np.int16)
    out = []
    for k in range(N):
        Y = np.clip(base + 8 * k + rng.integers(-4, 5, size=base.shape, dtype=np.int16), 16, 235).astype(np.uint8)
        U = np.clip(cbase + 2 * k + rng.integers(-3, 4, size=cbase.shape, dtype=np.int16), 16, 240).astype(np.uint8)
        V = np.clip(256 - cbase - 3 * k, 16, 240).astype(np.uint8)
        out.append((Y, U, V))
    return out


def widen(planes, rng):
    """the same picture at 10 bits, its two new low bits seeded"""
    return tuple((p.astype(np.uint16) << 2) | rng.integers(0, 4, size=p.shape, dtype=np.uint16) for p in planes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"frames_per_call": N, "width": W, "height": H, "subsampling": "420", "rounds": a.rounds, "calls_per_window": a.calls}
    with gs360.Context(device=0, n_slots=1) as ctx:
        res["device"] = ctx.info()["name"]
        host8 = frames8()
        rng = np.random.default_rng(2810)
        first10 = widen(host8[0], rng)
        planes = {8: [[ctx.to_device(p) for p in f] for f in host8],
                  10: [[ctx.to_device(p) for p in (first10 if k == 0 else widen(f, rng))] for k, f in enumerate(host8)]}
        del host8
        stages, jobs, dsts, ms = {}, {}, {}, {}
        for depth, out_bits in PAIRS:
            stages[depth, out_bits] = vidcolor.VideoColor(depth, out_bits=out_bits)
            dsts[depth, out_bits] = [ctx.alloc(H * W * 3 * (out_bits // 8)) for _ in range(N)]
            jobs[depth, out_bits] = [(p[0], p[1], p[2], W, H, "420", d) for p, d in zip(planes[depth], dsts[depth, out_bits])]
            ms[depth, out_bits] = []

        def window(pair, calls):
            ctx.event_record(0, 0)
            for _ in range(calls):
                stages[pair].convert_dev(ctx, jobs[pair])
            ctx.event_record(0, 1)
            ctx.sync(0)
            return ctx.event_elapsed_ms(0, 0, 1) / calls
        for pair in PAIRS:
            window(pair, 3)
        for _ in range(a.rounds):
            for pair in PAIRS:
                ms[pair].append(window(pair, a.calls))
        got = ctx.download(dsts[10, 8][0], (H, W, 3), dtype=np.uint8)
        res["d10_o8_equals_numpy_restatement"] = bool(np.array_equal(got, feed_ref.convert(*first10, "420")))
        for depth, out_bits in PAIRS:
            v = np.array(ms[depth, out_bits]) * 1e3 / N              # microseconds per frame, one value per window
            read, written = H * W * (depth > 8 and 2 or 1) * 1.5, H * W * 3 * (out_bits // 8)
            res[f"d{depth}_o{out_bits}"] = {"us_per_frame_median": float(np.median(v)), "us_per_frame_min": float(v.min()),
                                           "us_per_frame_max": float(v.max()), "bytes_read_per_frame": read,
                                           "bytes_written_per_frame": written,
                                           "gb_per_s_at_median": (read + written) / (float(np.median(v)) * 1e-6) / 1e9}
            stages[depth, out_bits].close()
    print(json.dumps(res, sort_keys=True))
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
