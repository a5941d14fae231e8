"""Voxel downsampling of a resident cloud (gs360/pointcloud.py, VOX-SPEC v1) on the MI355X against the NumPy restatement
(tests/voxel_np.py) on the same host.

Workload: one synthetic cloud of `--points` (default 20 M) float32 points, surface-like: 48 planar patches of random pose and size
(2 to 12 units across, 2 cm of noise off the plane) and 16 ellipsoid shells, the points dealt evenly to them and shuffled.  It is
uploaded once.  The voxel size timed is the one `voxel_downsample_to_target` finds for a 10 % target.

Device: the bounds, count and pick (centroid, first) calls, each HBM-cold (a 1 GiB buffer is rewritten before every timed call,
more than the 256 MiB Infinity Cache) and each timed by a host clock around the call, which returns after its own stream
synchronise; `--reps` calls each, alternating, after a warm-up.  Host: one np.unique(axis=0) probe over the int64 key triples (what
the reference runs per probe) and one pick of the restatement, wall time, once each.  End to end: voxel_downsample_to_target for
the 10 % target on the resident cloud, its log kept, with the number of device probes.

    python tests/tools/bench_voxel.py [--points 20000000] [--reps 7] [--no-host] [--out FILE]     (prints one JSON object)
"""
import argparse
import contextlib
import io
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[2]
for p in (str(ROOT / "360cam-pgm-3dgs-tools_amd"), str(ROOT / "tests")):
    sys.path.insert(0, p)

import gs360  # noqa: E402
import voxel_np  # noqa: E402
from gs360 import pointcloud  # noqa: E402


def surface_cloud(n, seed=2026):
    rng = np.random.default_rng(seed)
    parts, per = [], n // 64
    for s in range(64):
        m = per if s < 63 else n - 63 * per
        centre = rng.uniform(-40.0, 40.0, 3) * np.array([1.0, 1.0, 0.15])
        if s < 48:                                         # a planar patch
            q, _r = np.linalg.qr(rng.normal(size=(3, 3)))
            local = np.stack([rng.uniform(-1, 1, m) * rng.uniform(1.0, 6.0), rng.uniform(-1, 1, m) * rng.uniform(1.0, 6.0),
                              rng.normal(size=m) * 0.02], axis=1)
            pts = local @ q.T + centre
        else:                                              # an ellipsoid shell
            d = rng.normal(size=(m, 3))
            pts = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 4.0, 3) + rng.normal(size=(m, 3)) * 0.02 + centre
        parts.append(pts.astype(np.float32))
    xyz = np.concatenate(parts)
    return xyz[rng.permutation(n)]


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


def bench(n, reps, host=True):
    xyz = surface_cloud(n)
    rgb = np.zeros((n, 3), np.uint8)
    out = {"points": n, "reps": reps}
    with gs360.Context(device=0, n_slots=1) as ctx:
        flush = ctx.alloc(1 << 30)
        (cloud), out["upload_and_bounds_s"] = wall(lambda: pointcloud.Cloud(ctx, xyz))
        text = io.StringIO()
        with contextlib.redirect_stdout(text):
            res, out["to_target_10pct_s"] = wall(lambda: pointcloud.voxel_downsample_to_target(xyz, rgb, n // 10, return_indices=True, cloud=cloud))
        log = text.getvalue().splitlines()
        out["to_target_log"] = log
        out["to_target_probes"] = sum(ln.startswith(("[shrink", "[expand]", "[iter")) for ln in log) + 1
        voxel = float(next(ln for ln in log if ln.startswith("[final]")).split("voxel=")[1].split()[0])
        out["voxel"], out["voxels_at_it"] = voxel, int(res[2].shape[0])
        cloud.downsample_by_size(voxel, "centroid")      # the output buffers exist before the timed calls
        calls = {"bounds": lambda: ctx.cloud_bounds_dev(cloud.d_xyz, n, cloud.scratch),
                 "count": lambda: cloud.unique_count(voxel),
                 "pick_centroid": lambda: ctx.voxel_pick_dev(cloud.d_xyz, n, cloud.minmax, voxel, gs360.capi.VOXEL_CENTROID, cloud.scratch, cloud._out[0]),
                 "pick_first": lambda: ctx.voxel_pick_dev(cloud.d_xyz, n, cloud.minmax, voxel, gs360.capi.VOXEL_FIRST, cloud.scratch, cloud._out[0])}
        times = {name: [] for name in calls}
        for k in range(reps + 2):                          # two warm-up rounds
            for name, call in calls.items():
                ctx.memset(flush, k & 0xFF)
                ctx.sync(0)
                _r, dt = wall(call)
                if k >= 2:
                    times[name].append(dt * 1e3)
        out["device_ms"] = {name: {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))} for name, t in times.items()}
        minmax = cloud.minmax.copy()
        got = cloud.downsample_by_size(voxel, "centroid")
        cloud.close()
        ctx.free(flush)
    if not host:
        return out
    (count), out["host_unique_probe_s"] = wall(lambda: int(np.unique(voxel_np.triple_keys(xyz, minmax, voxel), axis=0).shape[0]))
    (want), out["host_restatement_pick_s"] = wall(lambda: voxel_np.pick(xyz, voxel, "centroid", minmax))
    out["count_equal"], out["pick_equal"] = bool(count == got.shape[0]), bool(np.array_equal(want, got))
    out["count_speedup_over_np_unique"] = out["host_unique_probe_s"] * 1e3 / out["device_ms"]["count"]["median"]
    out["pick_speedup_over_restatement"] = out["host_restatement_pick_s"] * 1e3 / out["device_ms"]["pick_centroid"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-host", action="store_true", help="device calls only (a run under a profiler)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = bench(a.points, a.reps, not a.no_host)
    print(json.dumps(res, sort_keys=True))
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
