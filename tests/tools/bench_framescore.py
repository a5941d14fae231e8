"""Frame sharpness statistics (gs360_frame_stats_u8) on the MI355X: 16 distinct 8K RGB frames per launch, HBM-cold (a 1 GiB
buffer is rewritten between timed launches, more than the 256 MiB Infinity Cache), metric lapvar (statistics only) and hybrid
(+ the INTER_AREA fft input), and a 3840 x 3840 fisheye pair with the circle mask.  Device-event times; the bytes every launch
must read (H * W * 3 per frame) over 8 TB/s give the share of the HBM roofline.  Also: the host FFT per frame (NumPy, the
reference's own code) and the NumPy restatement of the statistics as the CPU baseline.

    python tests/tools/bench_framescore.py [--reps 10] [--out FILE]     (prints one JSON object)
"""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[2]
for p in (str(ROOT / "360cam-pgm-3dgs-tools_amd"), str(ROOT / "tests")):
    sys.path.insert(0, p)

import gs360  # noqa: E402
from gs360 import capi, framescore  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def _time_launch(ctx, call, flush, reps):
    """median device time (ms) of call() over reps HBM-cold launches"""
    times = []
    for _ in range(reps):
        ctx.memset(flush, reps & 0xFF)
        ctx.event_record(0, 0)
        call()
        ctx.event_record(0, 1)
        times.append(ctx.event_elapsed_ms(0, 0, 1))
    return float(np.median(times)), float(min(times)), float(max(times))


def bench(reps):
    rng = np.random.default_rng(2026)
    out = {}
    with gs360.Context(device=0, n_slots=1) as ctx:
        flush = ctx.alloc(1 << 30)
        H, W = 3840, 7680
        base = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        frames = [ctx.to_device(np.roll(base, 131 * k, axis=1)) for k in range(16)]
        band = framescore.band_rows(H, 0.8)
        sw, sh = framescore.fft_input_size(W, band[1] - band[0])
        stats = ctx.alloc(16 * 104)
        smalls = [ctx.alloc(2 * sw * sh * 4) for _ in range(16)]
        for metric, sm in (("lapvar", None), ("hybrid", smalls)):
            def call():
                ctx.frame_stats_dev(frames, H, W, 3, band, stats, flags=capi.FS_HIGHLIGHTS, smalls=sm, small_w=sw, small_h=sh)
            call()
            ctx.sync(0)
            med, lo, hi = _time_launch(ctx, call, flush, reps)
            us = med * 1e3 / 16
            out[f"8k_{metric}"] = {"frames": 16, "ms_per_launch_median": med, "ms_min": lo, "ms_max": hi, "us_per_frame": us,
                                   "bytes_per_frame": H * W * 3, "roofline_fraction": (H * W * 3 / HBM_BYTES_PER_S) / (us * 1e-6)}
        # end-to-end host API on the resident frames (download of the records and fft inputs, host finish with the FFT)
        dframes = [framescore.DeviceFrame(b, H, W, 3) for b in frames]
        framescore.score_arrays(ctx, dframes, "hybrid", 0.8, True, True)
        t0 = time.perf_counter()
        framescore.score_arrays(ctx, dframes, "hybrid", 0.8, True, True)
        out["8k_hybrid_score_arrays_ms_per_frame"] = (time.perf_counter() - t0) * 1e3 / 16
        small = ctx.download(smalls[0], (2, sh, sw), np.float32)
        t0 = time.perf_counter()
        for _ in range(20):
            framescore.fft_energy(small[0], None)
        out["host_fft_ms_per_frame"] = (time.perf_counter() - t0) * 1e3 / 20
        for b in frames + smalls + [stats]:
            ctx.free(b)
        # fisheye pair, 3840 x 3840, circle mask + highlights
        P = 3840
        pair = [ctx.to_device(rng.integers(0, 256, size=(P, P, 3), dtype=np.uint8)) for _ in range(2)]
        pband = framescore.band_rows(P, 0.8)
        pw, ph = framescore.fft_input_size(P, pband[1] - pband[0])
        pstats = ctx.alloc(2 * 104)
        psmall = [ctx.alloc(2 * pw * ph * 4) for _ in range(2)]

        def pcall():
            ctx.frame_stats_dev(pair, P, P, 3, pband, pstats, flags=capi.FS_CIRCLE | capi.FS_HIGHLIGHTS, smalls=psmall, small_w=pw,
                                small_h=ph)
        pcall()
        ctx.sync(0)
        med, lo, hi = _time_launch(ctx, pcall, flush, reps)
        out["pair_3840_hybrid_circle"] = {"frames": 2, "ms_per_launch_median": med, "us_per_frame": med * 1e3 / 2,
                                          "roofline_fraction": (P * P * 3 / HBM_BYTES_PER_S) / (med * 1e-3 / 2)}
        for b in pair + psmall + [pstats, flush]:
            ctx.free(b)
    import framescore_np as fnp
    t0 = time.perf_counter()
    fnp.frame_stats(base, *band, False, True)
    out["numpy_restatement_s_per_8k_frame"] = time.perf_counter() - t0
    out["reps"] = reps
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = bench(a.reps)
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
