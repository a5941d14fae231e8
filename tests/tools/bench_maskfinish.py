"""Mask finishing on the device (gs360_mask_finish_u8, MSK-SPEC v1): 16 resident 7680 x 3840 raw masks per call -- a crowd of filled discs
plus 1 % noise, each mask the first one rolled -- finished with the defaults (close 5, p 15, f 25) and with --mask-expand-mode percent
at 1.0 (p = 77), output kind "mask".

  device  one call over the 16 resident masks, HIP events around it, warm, median of `--reps` calls, per mask
  numpy   tests/maskfinish_np.py on the first mask, one thread, once per setting (host time, for scale; the device's output of that
          mask must equal it)

There is no cv2 here, hence no time of the reference's own calls.  The kernels' own times come from running the device part alone
under a kernel trace:  rocprofv3 --kernel-trace --stats -- python tests/tools/bench_maskfinish.py --device-only

    python tests/tools/bench_maskfinish.py [--reps 20] [--device-only] [--out FILE]
(prints one JSON object)
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
from gs360 import maskfinish  # noqa: E402

H, W, N = 3840, 7680, 16
SETTINGS = {"defaults_p15": maskfinish.Params(), "percent_p77": maskfinish.Params(expand_mode="percent", expand_percent=1.0)}


def crowd():
    rng = np.random.default_rng(20261020)
    m = (rng.random((H, W)) < 0.01).astype(np.uint8) * 255
    yy, xx = np.ogrid[:H, :W]
    for _ in range(40):
        cy, cx, r = rng.integers(H // 3, H), rng.integers(0, W), rng.integers(30, 260)
        m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 255
    return m


def bench(ctx, params, d_masks, first, reps, device_only):
    jobs, keep = maskfinish.build_jobs([(H, W)] * N, params)
    outs = [ctx.alloc(H * W) for _ in range(N)]
    for j, src, out in zip(jobs, d_masks, outs):
        j.src, j.dst = src.ptr, out.ptr
    scratch, counts = ctx.alloc(ctx.mask_finish_scratch(jobs)), ctx.alloc(4 * N)

    def call():
        ctx.event_record(0, 0)
        ctx.mask_finish_dev(jobs, scratch, counts)
        ctx.event_record(0, 1)
        return ctx.event_elapsed_ms(0, 0, 1)
    for _ in range(2):
        call()
    ms = [call() for _ in range(reps)]
    res = {"masks": N, "height": H, "width": W, "reps": reps, "expand_pixels": int(jobs[0].expand_kh // 2), "close": int(jobs[0].close_kh),
           "fuse": int(jobs[0].fuse), "device_ms_per_call_median": float(np.median(ms)), "device_ms_per_call_min": float(min(ms)),
           "device_ms_per_call_max": float(max(ms)), "device_ms_per_mask": float(np.median(ms)) / N,
           "set_pixels_first_mask": int(ctx.download(counts, (N,), np.uint32)[0])}
    if not device_only:
        import maskfinish_np as ref
        got = ctx.download(outs[0], (H, W))
        t0 = time.perf_counter()
        want, n = ref.finish(first, params)
        res["numpy_s_per_mask"] = time.perf_counter() - t0
        res["device_equals_numpy"] = bool(np.array_equal(got, want) and n == res["set_pixels_first_mask"])
        print(f"# {res['expand_pixels']}: numpy {res['numpy_s_per_mask']:.1f} s, equal {res['device_equals_numpy']}", file=sys.stderr, flush=True)
    for b in outs + [scratch, counts]:
        ctx.free(b)
    del keep
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--device-only", action="store_true", help="the device calls alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    first = crowd()
    res = {}
    with gs360.Context(device=0, n_slots=1) as ctx:
        res["device"] = ctx.info()["name"]
        d_masks = [ctx.to_device(np.roll(first, 97 * k, axis=1)) for k in range(N)]
        for name, params in SETTINGS.items():
            res[name] = bench(ctx, params, d_masks, first, a.reps, a.device_only)
    print(json.dumps(res, sort_keys=True))
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
