"""gs360_frame_stats_u16 against gs360_frame_stats_u8 on the MI355X (FS-DEPTH16 v1): sixteen distinct 7680 x 3840 x 3 frames
resident in HBM per launch, statistics only (metric lapvar) and with the fft input (hybrid).  The two forms are timed in turn in one
process, HBM-cold (a 1 GiB buffer is rewritten before every timed launch, more than the 256 MiB Infinity Cache), with device events;
the bytes a launch must read (H * W * 3 samples per frame) over 8 TB/s give the share of the HBM roofline.  The 16-bit records of
frame 0 are checked against the int64 model at this size before anything is timed.

    python tests/tools/bench_framescore16.py [--reps 20] [--out FILE]     (prints one JSON object)
"""
import argparse
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[2]
for p in (str(ROOT / "360cam-pgm-3dgs-tools_amd"), str(ROOT / "tests")):
    sys.path.insert(0, p)

import gs360  # noqa: E402
from gs360 import capi, framescore  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
H, W, N = 3840, 7680, 16


def bench(reps):
    import framescore16_np as fnp16
    rng = np.random.default_rng(2026)
    out = {"reps": reps, "frames": N, "frame": [H, W, 3]}
    with gs360.Context(device=0, n_slots=1) as ctx:
        flush = ctx.alloc(1 << 30)
        base16 = rng.integers(0, 65536, size=(H, W, 3), dtype=np.uint16)
        frames = {16: [ctx.to_device(np.roll(base16, 131 * k, axis=1)) for k in range(N)],
                  8: [ctx.to_device(np.roll(base16 >> 8, 131 * k, axis=1).astype(np.uint8)) for k in range(N)]}
        band = framescore.band_rows(H, 0.8)
        sw, sh = framescore.fft_input_size(W, band[1] - band[0])
        stats = ctx.alloc(N * 104)
        smalls = [ctx.alloc(2 * sw * sh * 4) for _ in range(N)]

        def call(depth, sm):
            ctx.frame_stats_dev(frames[depth], H, W, 3, band, stats, flags=capi.FS_HIGHLIGHTS, smalls=sm, small_w=sw, small_h=sh,
                                depth=depth)
        call(16, None)
        ctx.sync(0)
        got = dict(zip(framescore.FIELDS, map(int, ctx.download(stats, (N, 13), np.int64)[0])))
        want = fnp16.frame_stats(base16, *band, False, True)
        if got != want:
            raise AssertionError(f"gs360_frame_stats_u16 differs from the model at {W} x {H}: {got} != {want}")
        out["records_equal_the_model_at_this_size"] = True
        for metric, sm in (("lapvar", None), ("hybrid", smalls)):
            times = {8: [], 16: []}
            for depth in (8, 16):
                call(depth, sm)                                 # warm-up of each shape
            ctx.sync(0)
            for _ in range(reps):
                for depth in (8, 16):                           # the two forms in turn
                    ctx.memset(flush, 0x3C)
                    ctx.event_record(0, 0)
                    call(depth, sm)
                    ctx.event_record(0, 1)
                    times[depth].append(ctx.event_elapsed_ms(0, 0, 1))
            for depth in (8, 16):
                t = np.array(times[depth])
                nbytes = H * W * 3 * (depth // 8)
                us = float(np.median(t)) * 1e3 / N
                out[f"{metric}_u{depth}"] = {"ms_per_launch_median": float(np.median(t)), "ms_min": float(t.min()), "ms_max": float(t.max()),
                                            "us_per_frame": us, "bytes_per_frame": nbytes, "tb_per_s": nbytes / (us * 1e-6) / 1e12,
                                            "roofline_fraction": (nbytes / HBM_BYTES_PER_S) / (us * 1e-6)}
            out[f"{metric}_u16_over_u8"] = out[f"{metric}_u16"]["ms_per_launch_median"] / out[f"{metric}_u8"]["ms_per_launch_median"]
        for b in frames[8] + frames[16] + smalls + [stats, flush]:
            ctx.free(b)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = bench(a.reps)
    print(json.dumps(res, sort_keys=True))
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
