"""Device JPEG encode (gs360_jpeg_scan_u8, JPG-SPEC v1) against Pillow on the same views, same host, same run: 12 x 1600^2 views of
a photo-like 8K frame (the full360coverage preset's geometry) are rendered once; then

  device  one call over the 12 resident views, HIP events around it, warm, median of `--reps` runs (>= 20), per view; the transfer
          the engine then makes (lengths, then the scans' bytes, into pinned memory) is timed separately with a host clock
  pillow  quality=100, subsampling=0, optimize=True and optimize=False on the downloaded arrays: one thread per view on
          `--threads` threads (16: the CPUs a job gets), wall time of the batch per view, and one view on one thread

and the stream bytes of the three are reported side by side.

    python tests/tools/bench_jpegenc.py [--reps 30] [--threads 16] [--quality 100] [--out FILE]     (prints one JSON object)
"""
import argparse
import io
import json
import pathlib
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[2]
for p in (str(ROOT / "360cam-pgm-3dgs-tools_amd"), str(ROOT / "tests")):
    sys.path.insert(0, p)

import gs360  # noqa: E402
from gs360 import jpegenc  # noqa: E402

SIZE = 1600
RESTART = 8


def synth(h, w, k=0):
    """gradients + a 64-pixel checker + 3 bits of hashed noise (scripts/bench_cli_e2e.py's frames)"""
    x = np.arange(w, dtype=np.uint32)[None, :]
    y = np.arange(h, dtype=np.uint32)[:, None]
    n = (((x * np.uint32(2654435761)) ^ (y * np.uint32(40503 + 977 * k))) >> np.uint32(29)).astype(np.uint8)
    img = np.empty((h, w, 3), np.uint8)
    img[..., 0] = ((x * 255) // w).astype(np.uint8) + n
    img[..., 1] = ((y * 255) // h).astype(np.uint8) + n
    img[..., 2] = ((((x >> 6) + (y >> 6)) & 1) * 96).astype(np.uint8) + n
    return img


def pillow_bytes(a, quality, optimize):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", quality=quality, subsampling=0, optimize=optimize)
    return b.tell()


def bench(reps, threads, quality):
    views = [gs360.View.make(90.0 * i, 0.0, 104.25, 104.25, SIZE, SIZE) for i in range(4)]
    views += [gs360.View.make(45 + 90.0 * i, p, 104.25, 104.25, SIZE, SIZE) for i in range(4) for p in (30.0, -30.0)]
    n, raw = len(views), SIZE * SIZE * 3
    with gs360.Context(device=0, n_slots=1) as ctx:
        d_src = ctx.to_device(synth(3840, 7680))
        d_views = [ctx.alloc(raw) for _ in views]
        ctx.equirect_views_dev([d_src], 7680, 3840, 3, views, d_views)
        ctx.sync(0)
        arrays = [ctx.download(d, (SIZE, SIZE, 3)) for d in d_views]
        d_out = [ctx.alloc(raw) for _ in views]
        d_len = ctx.alloc(8 * n)
        pinned = [ctx.pinned(raw) for _ in views]
        jobs = [(d, SIZE, SIZE, 3, 0, o, raw) for d, o in zip(d_views, d_out)]

        def encode():
            ctx.event_record(0, 0)
            ctx.jpeg_scan_dev(jobs, d_len, quality=quality, restart=RESTART)
            ctx.event_record(0, 1)
            return ctx.event_elapsed_ms(0, 0, 1)
        for _ in range(3):
            encode()
        ms = [encode() for _ in range(max(20, reps))]
        lengths = [int(v) for v in ctx.download(d_len, (n,), np.uint64)]
        assert max(lengths) <= raw, "a scan did not fit the view's raw size"
        xfer = []
        for _ in range(5):                              # what the engine does after the call: lengths, then the scans' bytes
            t0 = time.perf_counter()
            got = ctx.download(d_len, (n,), np.uint64)
            for hb, o, length in zip(pinned, d_out, got):
                gs360.capi._check(ctx.L.gs360_download(ctx.handle, hb.ptr, o.ptr, int(length), 0), ctx.L)
            ctx.sync(0)
            xfer.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        for d in d_views:                               # the pixel download it replaces
            gs360.capi._check(ctx.L.gs360_download(ctx.handle, pinned[0].ptr, d.ptr, raw, 0), ctx.L)
        ctx.sync(0)
        pixel_ms = (time.perf_counter() - t0) * 1e3
        head = len(jpegenc.header(SIZE, SIZE, 3, quality, RESTART)) + 2
        name = ctx.info()["name"]
        for hb in pinned:
            ctx.unpin(hb)
    out = {"device": name, "views": n, "size": SIZE, "quality": quality, "restart_interval": RESTART, "reps": len(ms),
           "device_ms_per_call_median": float(np.median(ms)), "device_ms_per_call_min": float(min(ms)), "device_ms_per_call_max": float(max(ms)),
           "device_ms_per_view": float(np.median(ms)) / n, "device_file_bytes_per_view": float(np.mean(lengths)) + head,
           "scan_download_ms_per_view": float(np.median(xfer)) / n, "pixel_download_ms_per_view": pixel_ms / n, "raw_bytes_per_view": raw}
    for key, optimize in (("pillow_optimize", True), ("pillow_plain", False)):
        t0 = time.perf_counter()
        one = pillow_bytes(arrays[0], quality, optimize)
        single = (time.perf_counter() - t0) * 1e3
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            with ThreadPoolExecutor(max_workers=threads) as pool:
                sizes = list(pool.map(lambda a: pillow_bytes(a, quality, optimize), arrays))
            walls.append((time.perf_counter() - t0) * 1e3)
        out[key] = {"ms_one_view_one_thread": single, "ms_per_view_batch_of_12": float(np.median(walls)) / n, "threads": threads,
                    "file_bytes_per_view": float(np.mean(sizes)), "first_view_bytes": one}
        out[key]["device_bytes_over_pillow"] = out["device_file_bytes_per_view"] / out[key]["file_bytes_per_view"]
        out[key]["pillow_ms_over_device_ms"] = out[key]["ms_per_view_batch_of_12"] / out["device_ms_per_view"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--quality", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = bench(a.reps, a.threads, a.quality)
    print(json.dumps(res, sort_keys=True))
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
