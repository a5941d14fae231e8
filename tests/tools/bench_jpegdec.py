"""Device JPEG decode (gs360_jpeg_decode_u8, JPD-SPEC v1) against Pillow on the same files, same host, same run: 16 distinct 7680 x 3840
quality-92 JPEGs of photo-like frames, 4:2:0 unless --subsampling (Pillow's numbers and the binding's) says otherwise.

  device  one call over the 16 files (scans, tables and segment records uploaded before), HIP events around it, warm, median of
          `--reps` runs, per frame.  The 16 frames' scratch and outputs are some gigabytes, far beyond the caches, so every run reads
          its inputs from HBM.  The rounds the entropy stage needed to settle its entry states across workgroups are reported per
          file.  The split by stage comes from the kernels' own times: run this tool under `rocprofv3 --kernel-trace --stats` and add
          up jd_sync_kernel + jd_chain_kernel + jd_write_kernel (entropy), jd_dc_kernel + jd_dc_carry_kernel (DC prediction) and
          jd_pixels_kernel (reconstruction).
  pillow  np.asarray(Image.open(...)) of the same bytes, one thread, median per frame
  pcie    bytes per frame that cross PCIe each way on the two paths

--subsampling 2 (4:2:0, the default), 0 (4:4:4) and 1 (4:2:2) are written by Pillow.  3 (4:4:0) and 4 (4:1:1) are written by the NumPy
writer of tests/jpegsamp_np.py, which is far too slow for whole 8K frames: it codes eight MCU rows of the first frame, each as one
restart interval, and every frame is those eight intervals over and over, frame k starting with row k.  Such a file has a restart
interval of one MCU row whatever --restart says (give a Pillow-written layout --restart = its MCUs per row to compare like with
like), and its bytes per frame are those of eight rows, repeated.  The result names the layout when it is not the default.

    python tests/tools/bench_jpegdec.py [--subsampling 2] [--reps 20] [--frames 16] [--width 7680] [--restart 0] [--out FILE]
    (prints one JSON object)
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


WRITTEN = {3: (1, 2), 4: (4, 1)}      # --subsampling -> luma sampling of the layouts Pillow does not write


def written_frames(frames, height, width, hs, vs):
    """-> [file bytes]: see the module docstring"""
    import jpegsamp_np as samp
    rows, mw, mh = 8, -(-width // (8 * hs)), -(-height // (8 * vs))
    z = samp.coefficients(synth(rows * 8 * vs, width), hs, vs, 92)
    intervals = [samp.scan(z[r * mw:(r + 1) * mw], hs, vs, 0) for r in range(rows)]
    head = samp.header(height, width, hs, vs, 92, mw)
    out = []
    for k in range(frames):
        body = b"".join(intervals[(k + r) % rows] + (bytes([0xFF, 0xD0 + (r & 7)]) if r + 1 < mh else b"") for r in range(mh))
        out.append(head + body + b"\xff\xd9")
    return out


def pillow_frames(frames, height, width, subsampling, restart):
    from PIL import Image
    out = []
    for k in range(frames):
        b = io.BytesIO()
        kw = {"restart_marker_blocks": restart} if restart else {}
        Image.fromarray(synth(height, width, k)).save(b, "JPEG", quality=92, subsampling=subsampling, **kw)
        out.append(b.getvalue())
    return out


def bench(reps, frames, width, restart, subsampling=2):
    from PIL import Image
    height = width // 2
    if subsampling in WRITTEN:
        files = written_frames(frames, height, width, *WRITTEN[subsampling])
    else:
        files = pillow_frames(frames, height, width, subsampling, restart)
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
        **({} if subsampling == 2 else {"subsampling": subsampling}),
        "frames": frames, "width": width, "height": height, "restart": d.restart if subsampling in WRITTEN else restart, "reps": reps,
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
    ap.add_argument("--subsampling", type=int, default=2, choices=(0, 1, 2, 3, 4))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--width", type=int, default=7680)
    ap.add_argument("--restart", type=int, default=0)
    ap.add_argument("--out")
    a = ap.parse_args()
    res = bench(a.reps, a.frames, a.width, a.restart, a.subsampling)
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).write_text(line + "\n")
