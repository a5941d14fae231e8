"""Device JPEG decode (gs360_jpeg_decode_u8, JPD-SPEC v1) against Pillow on the same files, same host, same run: 16 distinct 7680 x 3840
4:2:0 quality-92 JPEGs of photo-like frames.

  device  one call over the 16 files (scans, tables and segment records uploaded before), HIP events around it, warm, median of
          `--reps` runs, per frame.  The 16 frames' scratch and outputs are some gigabytes, far beyond the caches, so every run reads
          its inputs from HBM.  The rounds the entropy stage needed to settle its entry states across workgroups are reported per
          file.  The split by stage comes from the kernels' own times: run this tool under `rocprofv3 --kernel-trace --stats` and add
          up jd_sync_kernel + jd_chain_kernel + jd_write_kernel (entropy), jd_dc_kernel + jd_dc_carry_kernel (DC prediction) and
          jd_pixels_kernel (reconstruction).
  pillow  np.asarray(Image.open(...)) of the same bytes, one thread, median per frame
  pcie    bytes per frame that cross PCIe each way on the two paths

    python tests/tools/bench_jpegdec.py [--reps 20] [--frames 16] [--width 7680] [--restart 0] [--out FILE]     (prints one JSON object)
"""
import argparse
import io
import json
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[2]
for p in (str(ROOT / "360cam-pgm-3dgs-tools_amd"), str(ROOT / "tests")):
    sys.path.insert(0, p)

import gs360  # noqa: E402
from gs360 import jpegdec  # noqa: E402


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


def bench(reps, frames, width, restart):
    from PIL import Image
    height = width // 2
    files = []
    for k in range(frames):
        b = io.BytesIO()
        kw = {"restart_marker_blocks": restart} if restart else {}
        Image.fromarray(synth(height, width, k)).save(b, "JPEG", quality=92, subsampling=2, **kw)
        files.append(b.getvalue())
    pillow_ms = []
    for data in files:
        t0 = time.perf_counter()
        a = np.asarray(Image.open(io.BytesIO(data)))
        pillow_ms.append((time.perf_counter() - t0) * 1e3)
    want = a
    with gs360.Context(device=0, n_slots=1) as ctx:
        t0 = time.perf_counter()
        batch = jpegdec.Batch(ctx, files)
        prepare_ms = (time.perf_counter() - t0) * 1e3
        try:
            assert not batch.refused, batch.refused
            for _ in range(3):
                batch.run()
            assert batch.status() == [0] * frames
            ms = []
            for _ in range(reps):
                ctx.event_record(0, 0)
                batch.run()
                ctx.event_record(0, 1)
                ctx.sync(0)
                ms.append(ctx.event_elapsed_ms(0, 0, 1))
            rounds = batch.rounds()
            _k, d, b_out, _s, nscr, _stride = batch.items[-1]
            equal = bool(np.array_equal(ctx.download(b_out, (d.H, d.W, d.C)), want))
            uploaded = batch.uploaded
        finally:
            batch.close()
    raw = height * width * 3
    return {
        "frames": frames, "width": width, "height": height, "restart": restart, "reps": reps,
        "file_bytes_per_frame": int(np.mean([len(f) for f in files])),
        "device_ms_per_frame": statistics.median(ms) / frames, "device_ms_per_call_min": min(ms), "device_ms_per_call_max": max(ms),
        "chain_rounds": rounds, "last_frame_equals_pillow": equal,
        "host_parse_alloc_upload_ms_per_frame": prepare_ms / frames,
        "pillow_ms_per_frame_one_thread": statistics.median(pillow_ms),
        "pcie_bytes_per_frame": {"device_path_up": uploaded // frames, "device_path_down": 4, "host_path_up": raw, "host_path_down": 0},
        "scratch_bytes_per_frame": nscr,
    }


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--width", type=int, default=7680)
    ap.add_argument("--restart", type=int, default=0)
    ap.add_argument("--out")
    a = ap.parse_args()
    res = bench(a.reps, a.frames, a.width, a.restart)
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).write_text(line + "\n")
