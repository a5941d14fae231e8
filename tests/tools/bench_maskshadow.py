"""The shadow estimate on the device (gs360_mask_shadow_candidates_u8 and gs360_mask_shadow_merge_u8, MSK-SHADOW v1): 16 resident
7680 x 3840 images per call -- tests/maskshadow_cases.py's synthetic photograph (textured ground, a person disc, a soft shadow with a
bright spot, a saturated patch, specks) at that size, each image the first one rolled -- with the reference's defaults (sigma 21:
169 taps, near 25 or more, min_area 160) after a close of 5.

  device  the two calls over the 16 resident images, HIP events around each, warm, median of `--reps` calls, per image
  numpy   tests/maskshadow_np.py on the first image, one thread, once (host time, for scale; the device's M of that image must
          equal it)

There is no cv2 here, hence no time of the reference's own calls.  The kernels' own times come from running the device part alone
under a kernel trace:  rocprofv3 --kernel-trace --stats -- python tests/tools/bench_maskshadow.py --device-only

    python tests/tools/bench_maskshadow.py [--reps 20] [--device-only] [--out FILE]
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
from gs360 import capi, maskfinish  # noqa: E402

import maskshadow_cases as cases  # noqa: E402

H, W, N = 3840, 7680, 16
PARAMS, SHADOW = maskfinish.Params(thresh=127), maskfinish.ShadowParams()


def bench(ctx, d_images, d_masks, first, reps, device_only):
    w = maskfinish.gaussian_weights(SHADOW.sigma)
    half, sdiv, cache = np.ascontiguousarray(w[len(w) // 2:]), maskfinish.sat_div_table(), {}
    outs = [ctx.alloc(H * W) for _ in range(N)]
    jobs = []
    for img, src, out in zip(d_images, d_masks, outs):
        j = capi.ShadowJob()
        j.H, j.W, j.thresh, j.image, j.src, j.dst = H, W, PARAMS.thresh, img.ptr, src.ptr, out.ptr
        j.radius, j.weights, j.sdiv = len(half) - 1, half.ctypes.data, sdiv.ctypes.data
        j.t, j.delta_min, j.sat_max, j.min_area = SHADOW.t, SHADOW.delta_min, SHADOW.sat_max, SHADOW.min_area
        maskfinish.set_element(j, "close", PARAMS.close, cache)
        jobs.append(j)
    scratch, counts = ctx.alloc(ctx.mask_shadow_scratch(jobs)), ctx.alloc(4 * N)

    def call():
        ctx.event_record(0, 0)
        ctx.mask_shadow_candidates_dev(jobs, scratch, counts)
        ctx.event_record(0, 1)
        person = ctx.download(counts, (N,), np.uint32)
        for j, n in zip(jobs, person):
            k, close_k = maskfinish.shadow_sizes(int(n), SHADOW.near_px)
            maskfinish.set_element(j, "near", k, cache)
            maskfinish.set_element(j, "sclose", close_k, cache)
            maskfinish.set_element(j, "open", 3, cache)
        ctx.event_record(0, 2)
        ctx.mask_shadow_merge_dev(jobs, scratch, counts)
        ctx.event_record(0, 3)
        ctx.sync(0)
        return ctx.event_elapsed_ms(0, 0, 1), ctx.event_elapsed_ms(0, 2, 3), int(person[0])
    for _ in range(2):
        call()
    ms = [call() for _ in range(reps)]
    cand, merge = np.array([m[0] for m in ms]), np.array([m[1] for m in ms])
    res = {"images": N, "height": H, "width": W, "reps": reps, "radius": int(jobs[0].radius), "near": int(jobs[0].near_kw),
           "shadow_close": int(jobs[0].sclose_kw), "person_pixels_first_image": ms[0][2],
           "candidates_ms_per_call_median": float(np.median(cand)), "candidates_ms_per_call_min": float(cand.min()),
           "candidates_ms_per_call_max": float(cand.max()), "candidates_ms_per_image": float(np.median(cand)) / N,
           "merge_ms_per_call_median": float(np.median(merge)), "merge_ms_per_call_min": float(merge.min()),
           "merge_ms_per_call_max": float(merge.max()), "merge_ms_per_image": float(np.median(merge)) / N,
           "scratch_bytes_per_image": int(scratch.nbytes // N),
           "set_pixels_first_image": int(ctx.download(counts, (N,), np.uint32)[0])}
    if not device_only:
        import maskshadow_np as ref
        got = ctx.download(outs[0], (H, W))
        t0 = time.perf_counter()
        want = ref.shadow(first[0], first[1], PARAMS, SHADOW)
        res["numpy_s_per_image"] = time.perf_counter() - t0
        res["device_equals_numpy"] = bool(np.array_equal(got, np.where(want["M"], 255, 0)) and want["count"] == res["set_pixels_first_image"])
        print(f"# numpy {res['numpy_s_per_image']:.1f} s, equal {res['device_equals_numpy']}", file=sys.stderr, flush=True)
    for b in outs + [scratch, counts]:
        ctx.free(b)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--device-only", action="store_true", help="the device calls alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    img, raw, _sat = cases.photograph(H, W, 20261020)
    print("# image built", file=sys.stderr, flush=True)
    with gs360.Context(device=0, n_slots=1) as ctx:
        res = {"device": ctx.info()["name"]}
        d_images = [ctx.to_device(np.roll(img, 97 * k, axis=1)) for k in range(N)]
        d_masks = [ctx.to_device(np.roll(raw, 97 * k, axis=1)) for k in range(N)]
        res["shadow"] = bench(ctx, d_images, d_masks, (img, raw), a.reps, a.device_only)
    print(json.dumps(res, sort_keys=True))
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
