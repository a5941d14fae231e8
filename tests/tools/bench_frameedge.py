"""Frame edge score (gs360_frame_edge_u8, FS-EDGE v1) on the MI355X against the frame statistics pass with lapvar's arguments
(gs360_frame_stats_u8, no fft input) on the same frames in the same process, the two alternating: 16 distinct resident 8K RGB
frames per launch, crop 0.8, HBM-cold (a 1 GiB buffer is rewritten between timed launches, more than the 256 MiB Infinity Cache),
device-event times.  A warm-up of both first, then `--repeats` blocks of `--reps` launches of each (about a second of kernel time
with the defaults); the spread of the block medians is the run-to-run noise the ratio has to be read against.  The bytes a launch
must read (band rows for the edge pass, every row for the statistics) over 8 TB/s give the share of the HBM roofline.

With --against LIB (another build of libgs360hip.so, e.g. the previous commit's) the statistics pass of the two builds is timed on
the same frames as well, alternating, with a host clock around launch + synchronise (each library has its own stream): the check
that a change to the shared strip code did not move the statistics pass.

    python tests/tools/bench_frameedge.py [--reps 60] [--repeats 5] [--against LIB] [--out FILE]     (prints one JSON object)
"""
import argparse
import ctypes as C
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
FRAMES = 16


def _timed(ctx, call, flush, k):
    ctx.memset(flush, k & 0xFF)
    ctx.event_record(0, 0)
    call()
    ctx.event_record(0, 1)
    return ctx.event_elapsed_ms(0, 0, 1)


def _summary(blocks, nbytes):
    """blocks: per repeat the list of launch times (ms) -> medians and their spread, per-frame time, share of the HBM roofline"""
    meds = [float(np.median(b)) for b in blocks]
    med = float(np.median(meds))
    us = med * 1e3 / FRAMES
    return {"ms_per_launch_median": med, "block_medians_ms": meds, "block_spread": (max(meds) - min(meds)) / med,
            "ms_min": float(min(map(min, blocks))), "ms_max": float(max(map(max, blocks))), "us_per_frame": us,
            "bytes_per_frame": nbytes, "roofline_fraction": (nbytes / HBM_BYTES_PER_S) / (us * 1e-6)}


def _other_stats_call(path, frames, H, W, band, stats):
    """-> call(): gs360_frame_stats_u8 (lapvar's arguments) + synchronise through another build of the library, on its own context"""
    lib = C.CDLL(str(path))
    vp, i, pvp = C.c_void_p, C.c_int, C.POINTER(C.c_void_p)
    lib.gs360_ctx_create.argtypes = [i, i, pvp]
    lib.gs360_sync.argtypes = [vp, i]
    lib.gs360_frame_stats_u8.argtypes = [vp, pvp, i, i, i, i, C.c_size_t, i, i, i, C.c_uint32, vp, pvp, i, i, i]
    handle = C.c_void_p()
    if lib.gs360_ctx_create(0, 1, C.byref(handle)) != 0:
        raise RuntimeError(f"{path}: gs360_ctx_create failed")
    fp = (C.c_void_p * len(frames))(*[b.ptr for b in frames])

    def call():
        rc = lib.gs360_frame_stats_u8(handle, fp, len(frames), H, W, 3, 0, 0, band[0], band[1], capi.FS_HIGHLIGHTS, stats.ptr, None, 0, 0, 0)
        if rc != 0 or lib.gs360_sync(handle, 0) != 0:
            raise RuntimeError(f"{path}: gs360_frame_stats_u8 failed ({rc})")
    return call


def _against(ctx, other, this, flush, reps, repeats):
    """host-clock block medians (ms) of the two builds' statistics pass, alternating, HBM-cold"""
    blocks = {"this": [], "other": []}
    for _ in range(repeats):
        cur = {"this": [], "other": []}
        for k in range(reps):
            for name, call in (("this", this), ("other", other)):
                ctx.memset(flush, k & 0xFF)
                ctx.sync(0)
                t0 = time.perf_counter()
                call()
                cur[name].append((time.perf_counter() - t0) * 1e3)
        for name in cur:
            blocks[name].append(float(np.median(cur[name])))
    return {"host_ms_block_medians": blocks, "this_over_other": float(np.median(blocks["this"]) / np.median(blocks["other"]))}


def bench(reps, repeats, against=None):
    rng = np.random.default_rng(2026)
    with gs360.Context(device=0, n_slots=1) as ctx:
        flush = ctx.alloc(1 << 30)
        H, W = 3840, 7680
        base = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        frames = [ctx.to_device(np.roll(base, 131 * k, axis=1)) for k in range(FRAMES)]
        eband = framescore.edge_band_rows(H, 0.8)
        sband = framescore.band_rows(H, 0.8)
        edge = ctx.alloc(FRAMES * capi.C.sizeof(capi.FrameEdge))
        stats = ctx.alloc(FRAMES * capi.C.sizeof(capi.FrameStats))
        calls = {"edge": lambda: ctx.frame_edge_dev(frames, H, W, 3, eband, edge),
                 "stats_lapvar": lambda: ctx.frame_stats_dev(frames, H, W, 3, sband, stats, flags=capi.FS_HIGHLIGHTS)}
        for k in range(3):                                # warm-up: code objects, the flush buffer's pages
            for call in calls.values():
                _timed(ctx, call, flush, k)
        ctx.sync(0)
        blocks = {name: [] for name in calls}
        for _ in range(repeats):
            cur = {name: [] for name in calls}
            for k in range(reps):
                for name, call in calls.items():          # alternating
                    cur[name].append(_timed(ctx, call, flush, k))
            for name in calls:
                blocks[name].append(cur[name])
        out = {"edge": _summary(blocks["edge"], (eband[1] - eband[0]) * W * 3),
               "stats_lapvar": _summary(blocks["stats_lapvar"], H * W * 3)}
        out["edge_over_stats"] = out["edge"]["ms_per_launch_median"] / out["stats_lapvar"]["ms_per_launch_median"]
        out["edge_over_stats_per_block"] = [e / s for e, s in zip(out["edge"]["block_medians_ms"], out["stats_lapvar"]["block_medians_ms"])]
        if against:
            stats2 = ctx.alloc(FRAMES * capi.C.sizeof(capi.FrameStats))
            other = _other_stats_call(against, frames, H, W, sband, stats2)

            def this():
                calls["stats_lapvar"]()
                ctx.sync(0)
            for _ in range(3):
                this()
                other()
            same = np.array_equal(ctx.download(stats, (FRAMES, 13), np.int64), ctx.download(stats2, (FRAMES, 13), np.int64))
            out["stats_against"] = dict(_against(ctx, other, this, flush, reps, repeats), library=str(against), records_equal=bool(same))
            ctx.free(stats2)
        for b in frames + [edge, stats, flush]:
            ctx.free(b)
    out.update(reps=reps, repeats=repeats, frames=FRAMES, size=[W, H], crop=0.8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--against", default=None, help="another build of libgs360hip.so to time the statistics pass against")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = bench(a.reps, a.repeats, a.against)
    print(json.dumps(res, sort_keys=True))
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
