"""The inpaint stage on the device (gs360_mask_inpaint_u8, MSK-INPAINT v1): 16 resident 1600 x 1600 views per call --
tests/maskshadow_cases.py's synthetic photograph at that size, each image the first one rolled -- whose fill masks are eight discs
that cover about a tenth of the image, at the reference's radius of 5.

  device  one call over the 16 resident images, HIP events around it, warm, median of `--reps` calls, per image.  A call fills its
          images in place, so every call starts from images uploaded again (outside the events).
  numpy   tests/maskinpaint_np.py on the first image, one thread, once (host time, for scale; the device's bytes of that image
          must equal it)

There is no cv2 here, hence no time of the reference's own call, and the stage is new, hence no time of an earlier version.  The
kernels' own times -- the split into distance (mi_cols, mi_rows), list (mi_scan, mi_scatter) and fill -- come from running the device
part alone under a kernel trace:  rocprofv3 --kernel-trace --stats -- python tests/tools/bench_maskinpaint.py --device-only

    python tests/tools/bench_maskinpaint.py [--reps 20] [--device-only] [--out FILE]
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

import maskinpaint_np as ref  # noqa: E402
import maskshadow_cases as cases  # noqa: E402

H, W, N = 1600, 1600, 16
DISC_R = 101                                             # eight discs of this radius: 10 % of 1600 x 1600
CENTRES = [(250, 300), (300, 1100), (700, 700), (800, 1400), (1100, 250), (1250, 950), (1450, 1450), (1500, 600)]


def bench(ctx, images, fill, reps, device_only):
    d_images = [ctx.to_device(im) for im in images]
    d_fills = [ctx.to_device(np.roll(fill, 97 * k, axis=1)) for k in range(N)]
    jobs = []
    for img, f in zip(d_images, d_fills):
        j = capi.InpaintJob()
        j.image, j.fill, j.H, j.W, j.radius = img.ptr, f.ptr, H, W, maskfinish.INPAINT_RADIUS
        jobs.append(j)
    scratch, levels = ctx.alloc(ctx.mask_inpaint_scratch(jobs)), ctx.alloc(4 * N)

    def call():
        for buf, im in zip(d_images, images):
            ctx.upload(buf, im)
        ctx.event_record(0, 0)
        ctx.mask_inpaint_dev(jobs, scratch, levels)
        ctx.event_record(0, 1)
        ctx.sync(0)
        return ctx.event_elapsed_ms(0, 0, 1)
    for _ in range(2):
        call()
    ms = np.array([call() for _ in range(reps)])
    K = ctx.download(levels, (N,), np.uint32)
    res = {"images": N, "height": H, "width": W, "reps": reps, "radius": maskfinish.INPAINT_RADIUS,
           "fill_pixels_first_image": int((fill > 0).sum()), "fill_fraction": float((fill > 0).mean()),
           "levels": int(K.max()), "launches_per_call": 4 + int(K.max()),
           "ms_per_call_median": float(np.median(ms)), "ms_per_call_min": float(ms.min()), "ms_per_call_max": float(ms.max()),
           "ms_per_image": float(np.median(ms)) / N, "scratch_bytes_per_image": int(scratch.nbytes // N)}
    if not device_only:
        got = ctx.download(d_images[0], (H, W, 3))
        t0 = time.perf_counter()
        want, Kw = ref.inpaint(images[0], fill > 0)
        res["numpy_s_per_image"] = time.perf_counter() - t0
        res["device_equals_numpy"] = bool(np.array_equal(got, want) and Kw == int(K[0]))
        print(f"# numpy {res['numpy_s_per_image']:.1f} s, equal {res['device_equals_numpy']}", file=sys.stderr, flush=True)
    for b in d_images + d_fills + [scratch, levels]:
        ctx.free(b)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--device-only", action="store_true", help="the device calls alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    img, _raw, _sat = cases.photograph(H, W, 20261021)
    fill = np.where(ref.discs(H, W, CENTRES, DISC_R), 255, 0).astype(np.uint8)
    print("# image built", file=sys.stderr, flush=True)
    with gs360.Context(device=0, n_slots=1) as ctx:
        res = {"device": ctx.info()["name"]}
        images = [np.ascontiguousarray(np.roll(img, 97 * k, axis=1)) for k in range(N)]
        res["inpaint"] = bench(ctx, images, fill, a.reps, a.device_only)
    print(json.dumps(res, sort_keys=True))
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
