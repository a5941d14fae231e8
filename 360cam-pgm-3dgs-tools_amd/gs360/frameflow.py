"""Optical-flow motion on the GPU: the FrameSelector's flow pass (FS-FLOW v1).

Drop-in seams of cli_tools/gs360_FrameSelector.py (FLOW_METHOD "lucas_kanade", the default):
  _compute_pair_flow_magnitude(prev_path, curr_path, crop_ratio, mask_mode="none")                FS:1283-1337
  _compute_record_flow_magnitude(prev_record, curr_record, crop_ratio)                           FS:1340-1361
  _compute_flow_magnitudes(records, flow_mag_arr, flow_crop_ratio, workers, label, limiter=None)  FS:1364-1423
The per-pixel work (gray, crop, INTER_AREA, mask, goodFeaturesToTrack, the pyramids, calcOpticalFlowPyrLK) runs in
gs360_frame_flow_u8; what is left here is the reference's crop and size expressions, its None / 9999.0 branches and the chain
logic over records.  flow_arrays is the batched entry on uint8 ndarrays or framescore.DeviceFrames: every frame is decoded and
uploaded once, and the device computes each frame's corners and pyramid once, even when the frame is in two pairs.

8-bit sources by default: 16-bit and float images raise Gs360Error (GS360_ERR_UNSUPPORTED), as scoring does.  With
GS360_FS_DEPTH16=device (FS-DEPTH16 v1) uint16 frames go through gs360_frame_flow_u16, which reads every sample's high byte, as
cv2.imread(IMREAD_GRAYSCALE) does of a 16-bit file, and is FS-FLOW v1 from there on.  The Farneback method is not implemented.
"""
import concurrent.futures
import math
import os
import sys
import threading

import numpy as np

from . import capi, framescore, imageio

FLOW_DOWNSCALE = 320              # FS:317
FLOW_MISSING_HIGH_VALUE = 9999.0  # FS:322
FLOW_CROP_RATIO = 0.6             # FS:323 (the main flow forces 1.0 for pair inputs, FS:2158-2163)
PROGRESS_INTERVAL = 5             # FS:332
RECORD_DTYPE = capi.record_dtype(capi.FrameFlow)
POINT_DTYPE = capi.record_dtype(capi.FlowPoint)
CHUNK_PAIRS = 32                  # record pairs per device call of _compute_flow_magnitudes

cancel_event = threading.Event()  # the reference's module-level cancel flag (FS:63)
_decode = framescore.decode       # the path-based seams' decode, looked up at call time so that tests can replace it


def flow_geometry(H, W, crop_ratio):
    """_load_flow_gray's crop and size (FS:1251-1270) -> (crop_x0, crop_y0, crop_w, crop_h, small_w, small_h)."""
    h, w = H, W
    x0 = y0 = 0
    if crop_ratio and 0.0 < crop_ratio < 1.0:
        ch = max(1, int(round(h * crop_ratio)))
        cw = max(1, int(round(w * crop_ratio)))
        y0 = max(0, (h - ch) // 2)
        x0 = max(0, (w - cw) // 2)
        h, w = min(ch, H - y0), min(cw, W - x0)
    sw, sh = w, h
    if FLOW_DOWNSCALE and max(h, w) > FLOW_DOWNSCALE:
        scale = FLOW_DOWNSCALE / float(max(h, w))
        sw, sh = max(1, int(w * scale)), max(1, int(h * scale))
    return x0, y0, w, h, sw, sh


def area_fast_factors(cw, ch, sw, sh):
    """(kx, ky) when cv2.resize INTER_AREA takes its integer-factor path for cw x ch -> sw x sh (1 / (dsize / ssize) an integer
    on both axes, to DBL_EPSILON, and the blocks tile the source), else None."""
    sx, sy = 1.0 / (sw / cw), 1.0 / (sh / ch)
    ix, iy = int(np.rint(sx)), int(np.rint(sy))
    eps = np.finfo(np.float64).eps
    if abs(sx - ix) < eps and abs(sy - iy) < eps and sw * ix == cw and sh * iy == ch:
        return ix, iy
    return None


def value_of(rec):
    """The reference's pair value from a record (n_corners, n_tracked, sum_mag): the mean magnitude, or None without corners,
    without a tracked point, or when it is not finite."""
    n_corners, n_tracked, sum_mag = (rec[k] for k in ("n_corners", "n_tracked", "sum_mag")) if not isinstance(rec, tuple) else rec
    if n_corners <= 0 or n_tracked <= 0:
        return None
    v = float(sum_mag) / float(n_tracked)
    return v if math.isfinite(v) else None


def _host_gray(fr, red_index):
    a = np.asarray(fr)
    if a.dtype == np.uint16:
        a = (a >> 8).astype(np.uint8)     # FS-DEPTH16 v1: the flow pass reads a 16-bit frame's 8-bit view
    if a.ndim == 2 or a.shape[2] == 1:
        return a.reshape(a.shape[0], a.shape[1])
    a = a.astype(np.int32)
    g = (a[:, :, red_index] * 4899 + a[:, :, 1] * 9617 + a[:, :, 2 - red_index] * 1868 + 8192) >> 14
    return g.astype(np.uint8)


def flow_records(ctx, frames, pairs, crop_ratio, mask_mode="none", red_index=0, with_points=False):
    """One gs360_frame_flow record per pair (a structured array of RECORD_DTYPE) for uint8 frames (H x W or H x W x C ndarrays, RGB(A)
    order unless red_index = 2, or framescore.DeviceFrames) and pairs of (prev, curr) indices into frames; a pair of frames of
    different sizes gets n_corners = -1.  Every DeviceFrame is read with its own row stride: pairs go to the device grouped by
    shape, kind and stride, and a pair of DeviceFrames of two strides runs on packed copies of both.  with_points: also the
    FlowPoint records, len(pairs) x FLOW_MAX_CORNERS (POINT_DTYPE)."""
    frames = list(frames)
    pairs = [(int(a), int(b)) for a, b in pairs]
    for a, b in pairs:
        if not (0 <= a < len(frames) and 0 <= b < len(frames)):
            raise IndexError(f"pair ({a}, {b}) outside the {len(frames)} frames")
    shapes = [framescore.frame_shape(fr) for fr in frames]   # 16-bit / float sources fail before any GPU work
    recs = np.zeros(len(pairs), RECORD_DTYPE)
    pts = np.zeros((len(pairs), capi.FLOW_MAX_CORNERS), POINT_DTYPE) if with_points else None
    ctx = ctx or framescore.default_context()
    flags = capi.FS_CIRCLE if mask_mode == "fisheye_circle" else 0
    depths = [framescore.frame_depth(fr) for fr in frames]
    groups = {}                           # (H, W, C, on device, row stride, which frames, depth) -> pair positions: one device call each
    gray = {}                             # frame index -> host gray, for pairs whose frames differ only in channels
    packed = {}                           # frame index -> packed host copy, for pairs of device frames of different row strides
    for k, (a, b) in enumerate(pairs):
        if shapes[a][:2] != shapes[b][:2]:
            recs[k]["n_corners"] = -1
            continue
        dev = isinstance(frames[a], framescore.DeviceFrame), isinstance(frames[b], framescore.DeviceFrame)
        strides = framescore.row_stride(frames[a]), framescore.row_stride(frames[b])
        if shapes[a] == shapes[b] and dev[0] == dev[1] and strides[0] == strides[1] and depths[a] == depths[b]:
            groups.setdefault(shapes[a] + (dev[0], strides[0], "own", depths[a]), []).append(k)
            continue
        if shapes[a] == shapes[b] and dev[0] and dev[1] and depths[a] == depths[b]:
            # the entry point takes one stride per call: such a pair (no producer makes one today) runs on packed copies
            for f in (a, b):
                if f not in packed:
                    packed[f] = framescore.host_copy(ctx, frames[f])
            groups.setdefault(shapes[a] + (False, shapes[a][1] * shapes[a][2] * (depths[a] // 8), "packed", depths[a]), []).append(k)
            continue
        # a device frame beside a host frame (a file the device JPEG decoder left to the host), or an 8-bit host frame beside a
        # 16-bit one: a packed 8-bit gray plane pairs with the host frame's gray (of its 8-bit view); any other device frame has no
        # host twin to convert
        if any(dv and (shapes[f][2] != 1 or depths[f] != 8 or frames[f].stride not in (0, shapes[f][1])) for f, dv in zip((a, b), dev)):
            raise ValueError("a pair of device frames must share the channel count and the sample type")
        for f, dv in zip((a, b), dev):
            if not dv:
                gray.setdefault(f, _host_gray(frames[f], red_index))
        groups.setdefault(shapes[a][:2] + (1, False, shapes[a][1], "gray", 8), []).append(k)
    for key, ks in groups.items():
        H, W, Cn = key[:3]
        use_gray = key[5] == "gray"
        idx = sorted({f for k in ks for f in pairs[k]})
        local = {f: i for i, f in enumerate(idx)}
        x0, y0, cw, ch, sw, sh = flow_geometry(H, W, crop_ratio)
        own = {"own": {}, "gray": gray, "packed": packed}[key[5]]
        with framescore.device_frames(ctx, [own.get(f, frames[f]) for f in idx]) as (bufs, stride, alloc):
            out = alloc(len(ks) * RECORD_DTYPE.itemsize)
            pbuf = alloc(len(ks) * capi.FLOW_MAX_CORNERS * POINT_DTYPE.itemsize) if with_points else None
            with ctx.slot_locks[0]:
                ctx.frame_flow_dev(bufs, H, W, Cn, (x0, y0, cw, ch), sw, sh, [(local[pairs[k][0]], local[pairs[k][1]]) for k in ks], out,
                                   flags=flags, points=pbuf, red_index=0 if use_gray else red_index, stride=stride, slot=0,
                                   **framescore.depth_keyword(key[6]))
                got = ctx.download(out, (len(ks),), RECORD_DTYPE)
                if with_points:
                    gp = ctx.download(pbuf, (len(ks), capi.FLOW_MAX_CORNERS), POINT_DTYPE)
        recs[ks] = got
        if with_points:
            pts[ks] = gp
    return (recs, pts) if with_points else recs


def flow_arrays(ctx, frames, pairs, crop_ratio, mask_mode="none", red_index=0):
    """The reference's pair value (_compute_pair_flow_magnitude, FS:1283-1323) for every (prev, curr) pair of frame indices: a
    float, or None (no corner, no tracked point, frames of different sizes).  frames: uint8 ndarrays or framescore.DeviceFrames;
    ctx None = the process's default context."""
    recs = flow_records(ctx, frames, pairs, crop_ratio, mask_mode, red_index)
    return [value_of(r) for r in recs]


def _compute_pair_flow_magnitude(prev_path, curr_path, crop_ratio, mask_mode="none"):
    """Drop-in for the reference's _compute_pair_flow_magnitude (FS:1283-1337, Lucas-Kanade) on the GPU."""
    with framescore._source(lambda p: _decode(p)) as src:
        read = (lambda p: src.read([p])[0]) if src else _decode
        a = read(prev_path)
        if a is None:
            return None
        b = read(curr_path)
        if b is None:
            return None
        return flow_arrays(None, [a, b], [(0, 1)], crop_ratio, mask_mode)[0]


def _record_exists(record):
    paths = record.get("file_paths", [])
    return bool(paths) and all(os.path.isfile(p) for p in paths)


def _compute_record_flow_magnitude(prev_record, curr_record, crop_ratio):
    """Drop-in for the reference's _compute_record_flow_magnitude (FS:1340-1361): the mean over the records' paths (X and Y of a
    pair record, with the circle mask)."""
    prev_paths = list(prev_record.get("file_paths", []))
    curr_paths = list(curr_record.get("file_paths", []))
    if not prev_paths or not curr_paths or len(prev_paths) != len(curr_paths):
        return None
    mask_mode = framescore.record_mask_mode(curr_record)
    return framescore.mean_finite([_compute_pair_flow_magnitude(p, c, crop_ratio, mask_mode=mask_mode)
                                   for p, c in zip(prev_paths, curr_paths)])


def update_progress(label, completed, total, last_pct):
    """The reference's progress line (FS:520-528)."""
    if total <= 0:
        return last_pct
    pct = int((completed * 100) / total)
    if last_pct < 0 or pct >= 100 or pct - last_pct >= PROGRESS_INTERVAL:
        sys.stdout.write(f"{label}... {pct:3d}% ({completed}/{total})\r")
        sys.stdout.flush()
        return pct
    return last_pct


def _chunk_values(ctx, records, chunk, images):
    """Record-pair values of one chunk of (left, right) record indices, from the decoded images {record index: [array or None]}."""
    jobs = {}      # mask_mode -> (frames, frame key -> index, pairs, [(chunk position, path index)])
    per = [[None] * len(records[r].get("file_paths", [])) for _, r in chunk]
    ok = []
    for pos, (l, r) in enumerate(chunk):
        lp, rp = images[l], images[r]
        good = len(lp) == len(rp) and len(lp) > 0
        ok.append(good)
        if not good:
            continue
        mode = framescore.record_mask_mode(records[r])
        frames, where, prs, dest = jobs.setdefault(mode, ([], {}, [], []))
        for j, (a, b) in enumerate(zip(lp, rp)):
            if a is None or b is None:
                continue
            ids = []
            for key, img in (((l, j), a), ((r, j), b)):
                if key not in where:
                    where[key] = len(frames)
                    frames.append(img)
                ids.append(where[key])
            prs.append(tuple(ids))
            dest.append((pos, j))
    return jobs, per, ok


def _compute_flow_magnitudes(records, flow_mag_arr, flow_crop_ratio, workers, label, limiter=None):
    """Drop-in for the reference's _compute_flow_magnitudes (FS:1364-1423): consecutive existing records form pairs (a missing
    record breaks the chain), each pair's value (9999.0 when None) raises both of its entries of flow_mag_arr in place, and the
    count of completed pairs is returned.  Every file is decoded once, on a thread pool that runs ahead of the GPU; the progress
    line is the reference's.  limiter: as the reference's, around each decode."""
    if len(records) < 2:
        return 0
    pair_indices = []
    prev_idx = None
    for idx, record in enumerate(records):
        if cancel_event.is_set():
            break
        if not _record_exists(record):
            prev_idx = None
            continue
        if prev_idx is not None:
            pair_indices.append((prev_idx, idx))
        prev_idx = idx
    total_pairs = len(pair_indices)
    if total_pairs == 0:
        return 0
    ctx = framescore.default_context()
    workers = max(1, min(16, int(workers or (os.cpu_count() or 1))))
    chunks = [pair_indices[i:i + CHUNK_PAIRS] for i in range(0, total_pairs, CHUNK_PAIRS)]

    def decode(path):
        if limiter is None:
            return _decode(path)
        limiter.acquire()
        try:
            return _decode(path)
        finally:
            limiter.release()

    completed = 0
    last_pct = -1
    with concurrent.futures.ThreadPoolExecutor(max_workers=workers) as ex, framescore._source(decode) as src:
        futs = {}
        resolved = {}                            # device decoder: record -> its frames, once the decode calls are queued

        def submit(chunk):
            for l, r in chunk:
                for k in (l, r):
                    if k not in futs:
                        futs[k] = [ex.submit(src.load if src else decode, p) for p in records[k].get("file_paths", [])]

        def frames_of(chunk):
            if not src:
                return {k: [f.result() for f in futs[k]] for lr in chunk for k in lr}
            new = [k for k in dict.fromkeys(k for lr in chunk for k in lr) if k not in resolved]
            flat = [(k, p, f.result()) for k in new for p, f in zip(records[k].get("file_paths", []), futs[k])]
            got = src.resolve([p for _, p, _ in flat], [item for _, _, item in flat])    # one run of decode calls for the chunk
            for k in new:
                resolved[k] = []
            for (k, _, _), fr in zip(flat, got):
                resolved[k].append(fr)
            return {k: resolved[k] for lr in chunk for k in lr}
        submit(chunks[0])
        for ci, chunk in enumerate(chunks):
            if cancel_event.is_set():
                break
            if ci + 1 < len(chunks):
                submit(chunks[ci + 1])           # decode ahead while this chunk runs on the GPU
            images = frames_of(chunk)
            jobs, per, ok = _chunk_values(ctx, records, chunk, images)
            for mode, (frames, _, prs, dest) in jobs.items():
                for (pos, j), v in zip(dest, flow_arrays(ctx, frames, prs, flow_crop_ratio, mode)):
                    per[pos][j] = v
            for pos, (l, r) in enumerate(chunk):
                mean_mag = framescore.mean_finite(per[pos]) if ok[pos] else None
                if mean_mag is None or not math.isfinite(mean_mag):
                    mean_mag = FLOW_MISSING_HIGH_VALUE
                flow_mag_arr[r] = max(flow_mag_arr[r], mean_mag)
                flow_mag_arr[l] = max(flow_mag_arr[l], mean_mag)
                completed += 1
                last_pct = update_progress(label, completed, total_pairs, last_pct)
            keep = {k for lr in (chunks[ci + 1] if ci + 1 < len(chunks) else []) for k in lr}
            for k in [k for k in futs if k not in keep]:
                del futs[k]                      # a record's images live until its last chunk
                if src:
                    src.release(resolved.pop(k, []))
    return completed
