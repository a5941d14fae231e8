"""Frame FFT energy (gs360_frame_fft_energy) on the MI355X.

- The FFT launch alone, 16 frames per launch, for the fft inputs of an 8K band at crop 0.8 (512 x 204) and of a 3840^2 fisheye
  pair frame (512 x 409): device-event medians, and the DFT's FLOPs (row pass 2 * 2 * h * w * (w/2+1), column pass 8 * h * h *
  (w/2+1)) over that time.
- score_arrays, metric hybrid, end to end on 16 resident 8K frames (DeviceFrames), fft="host" against fft="device", alternated.
- The precision sweep of FS-FFT v1: the worst |dev - ref| of the energy (both branches) against a float64 FFT over noise and
  photo-like inputs of several sizes, as a relative error, and where the reference is (about) zero -- constant inputs, or a mask
  that keeps only the donut's hole -- as an absolute error.

    python tests/tools/bench_framescore_fft.py [--reps 20] [--out FILE]     (prints one JSON object)
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
import framescore_fft_np as ffnp  # noqa: E402



def _planes(rng, h, w, kind):
    yy, xx = np.mgrid[:h, :w]
    if kind == "constant":
        g = np.full((h, w), 181.625, np.float32)
    elif kind == "noise":
        g = rng.uniform(0, 255, size=(h, w)).astype(np.float32)
    else:
        g = 60 + 0.3 * xx + 0.2 * yy + np.where(xx > w / 2, 70, 0) + rng.normal(0, 2, size=(h, w))
        g = np.clip(np.where((xx - w / 3) ** 2 + (yy - h / 2) ** 2 < (min(h, w) / 4) ** 2, 250, g), 0, 255).astype(np.float32)
    near = np.clip(np.round(g + rng.integers(-2, 3, size=(h, w))), 0, 255).astype(np.float32)
    return np.stack([g, near])


def _time_fft(ctx, h, w, H, W, band, flags, reps, rng):
    bufs = [ctx.to_device(_planes(rng, h, w, "photo")) for _ in range(16)]
    out = ctx.alloc(16 * framescore.FFT_DTYPE.itemsize)

    def call():
        ctx.frame_fft_energy_dev(bufs, w, h, H, W, band, out, flags=flags)
    call()
    ctx.sync(0)
    times = []
    for _ in range(reps):
        ctx.event_record(0, 0)
        call()
        ctx.event_record(0, 1)
        times.append(ctx.event_elapsed_ms(0, 0, 1))
    for b in bufs + [out]:
        ctx.free(b)
    med = float(np.median(times))
    K = w // 2 + 1
    flop = 16 * (4.0 * h * w * K + 8.0 * h * h * K)
    return {"h": h, "w": w, "frames": 16, "ms_per_launch_median": med, "ms_min": float(min(times)), "ms_max": float(max(times)),
            "us_per_frame": med * 1e3 / 16, "dft_gflop_per_frame": flop / 16 / 1e9, "tflops": flop / (med * 1e-3) / 1e12}


def _precision(ctx, rng):
    worst_rel, worst_abs_const, cases = 0.0, 0.0, 0
    for h, w in [(204, 512), (409, 512), (512, 512), (509, 127), (1, 512), (512, 1), (17, 3)]:
        H, W = 2 * h + 3, 3 * w + 1
        band = framescore.band_rows(H, 0.8)
        for kind in ("constant", "noise", "photo"):
            p = _planes(rng, h, w, kind)
            for flags in (0, capi.FS_CIRCLE | capi.FS_HIGHLIGHTS):
                b = ctx.to_device(p)
                out = ctx.alloc(framescore.FFT_DTYPE.itemsize)
                ctx.frame_fft_energy_dev([b], w, h, H, W, band, out, flags=flags)
                r = ctx.download(out, (1,), framescore.FFT_DTYPE)[0]
                ctx.free(b)
                ctx.free(out)
                rec = {f: r[f].item() for f in framescore.FFT_DTYPE.names}
                ref = ffnp.fft_record(p[0], p[1], H, W, band, flags)
                for masked in (False, True):
                    got, want = framescore.fft_energy_from_record(rec, masked), framescore.fft_energy_from_record(ref, masked)
                    err = abs(got - want)
                    if kind == "constant" or want == 0.0:     # (a mask can leave only the donut's hole valid)
                        worst_abs_const = max(worst_abs_const, err)
                    else:
                        worst_rel = max(worst_rel, err / want)
                    cases += 1
    return {"cases": cases, "worst_rel_err": worst_rel, "worst_abs_err_zero_reference": worst_abs_const}


def bench(reps):
    rng = np.random.default_rng(2026)
    out = {}
    with gs360.Context(device=0, n_slots=1) as ctx:
        band8 = framescore.band_rows(3840, 0.8)
        sw, sh = framescore.fft_input_size(7680, band8[1] - band8[0])
        out["fft_8k"] = _time_fft(ctx, sh, sw, 3840, 7680, band8, capi.FS_HIGHLIGHTS, reps, rng)
        bandp = framescore.band_rows(3840, 0.8)
        pw, ph = framescore.fft_input_size(3840, bandp[1] - bandp[0])
        out["fft_pair_3840"] = _time_fft(ctx, ph, pw, 3840, 3840, bandp, capi.FS_CIRCLE | capi.FS_HIGHLIGHTS, reps, rng)
        out["precision"] = _precision(ctx, rng)
        # end to end on 16 resident 8K frames, hybrid, the two fft paths alternated
        H, W = 3840, 7680
        base = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        bufs = [ctx.to_device(np.roll(base, 131 * k, axis=1)) for k in range(16)]
        frames = [framescore.DeviceFrame(b, H, W, 3) for b in bufs]
        t = {"host": [], "device": []}
        res = {}
        for mode in ("host", "device"):
            res[mode] = framescore.score_arrays(ctx, frames, "hybrid", 0.8, True, True, fft=mode)
        for _ in range(5):
            for mode in ("host", "device"):
                t0 = time.perf_counter()
                framescore.score_arrays(ctx, frames, "hybrid", 0.8, True, True, fft=mode)
                t[mode].append((time.perf_counter() - t0) * 1e3 / 16)
        for mode in ("host", "device"):
            out[f"8k_hybrid_score_arrays_{mode}_ms_per_frame"] = float(np.median(t[mode]))
        out["8k_hybrid_speedup"] = out["8k_hybrid_score_arrays_host_ms_per_frame"] / out["8k_hybrid_score_arrays_device_ms_per_frame"]
        out["8k_hybrid_max_rel_diff_sharp"] = max(abs(a[0] - b[0]) / abs(b[0]) for a, b in zip(res["device"], res["host"]))
        for b in bufs:
            ctx.free(b)
    out["reps"] = reps
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
