"""Adaptive octree sampling of a resident cloud (gs360/pointcloud.py, OCT-SPEC v1) on the MI355X, stage by stage, against the NumPy
restatement of the reference algorithm (tests/octree_np.py) on the same host.

Workload: bench_voxel.py's synthetic surface-like cloud of `--points` (default 20 M) float32 points, uploaded once.  Targets: 10 %
and 1 % of the cloud, and 8 -- the root's children, where one wavefront walks each leaf of millions of points.

Device: gs360_octree_pick_f32 with the centroid pick, each call HBM-cold (a 1 GiB buffer is rewritten before every timed call, more
than the 256 MiB Infinity Cache) and timed by a host clock around the call, which returns after its own stream synchronise; `--reps`
calls per target after a warm-up.  Then the same calls asking for the library's own stage clock (a host clock after a stream
synchronise behind every stage): codes, sort, levels, download, walk, ordinals, second sort, pick (with its download), selection.
Host: the restatement's pick at `--host-points` (default 2 M; it is the reference's algorithm, not its code, and far faster than the
reference's eight masks per split), wall time, once per target share.

    python tests/tools/bench_octree.py [--points 20000000] [--reps 7] [--host-points 2000000] [--out FILE]     (prints one JSON object)
"""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[2]
for p in (str(ROOT / "360cam-pgm-3dgs-tools_amd"), str(ROOT / "tests"), str(ROOT / "tests" / "tools")):
    sys.path.insert(0, p)

import gs360  # noqa: E402
import octree_np  # noqa: E402
from bench_voxel import surface_cloud, wall  # noqa: E402
from gs360 import pointcloud  # noqa: E402

STAGES = ("codes", "sort", "levels", "download", "walk", "ordinals", "second_sort", "pick", "select")


def spread(t):
    return {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}


def bench(n, reps, host_points):
    xyz = surface_cloud(n)
    out = {"points": n, "reps": reps, "targets": {}}
    with gs360.Context(device=0, n_slots=1) as ctx:
        flush = ctx.alloc(1 << 30)
        cloud = pointcloud.Cloud(ctx, xyz)
        scratch = ctx.alloc(ctx.octree_scratch(n))
        cube_min, cube_size = octree_np.cube(xyz)
        for name, target in (("10pct", n // 10), ("1pct", n // 100), ("8", 8)):
            res = {"target": target}
            for staged in (False, True):
                total, stages = [], []
                for k in range(reps + 1):                  # one warm-up round
                    ctx.memset(flush, k & 0xFF)
                    ctx.sync(0)
                    t0 = time.perf_counter()
                    picks, _s, _c, ms = ctx.octree_pick_dev(cloud.d_xyz, n, cube_min, cube_size, target, 1.0, 0.0, gs360.capi.VOXEL_CENTROID, scratch,
                                                            stages=staged)
                    if k:
                        total.append((time.perf_counter() - t0) * 1e3)
                        stages.append(ms)
                res["kept"] = int(picks.shape[0])
                if staged:
                    res["staged_call_ms"] = spread(total)
                    res["stage_ms"] = {s: spread([ms[i] for ms in stages]) for i, s in enumerate(STAGES)}
                else:
                    res["call_ms"] = spread(total)
            out["targets"][name] = res
        ctx.free(scratch)
        cloud.close()
        ctx.free(flush)
    if host_points:
        small = xyz[:host_points]
        out["host"] = {"points": int(small.shape[0])}
        for name, target in (("10pct", small.shape[0] // 10), ("1pct", small.shape[0] // 100), ("8", 8)):
            _picks, out["host"][f"restatement_{name}_s"] = wall(lambda: octree_np.pick(small, target))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-points", type=int, default=2_000_000, help="0: device calls only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = bench(a.points, a.reps, a.host_points)
    print(json.dumps(res, sort_keys=True))
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
