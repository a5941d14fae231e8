"""VID-FISHEYE v1 (gs360_video_fisheye_rgb) at the drop-in's defaults: 16 DISTINCT 3840 x 3840 4:2:0 fisheye
frames per call -> 16 views of 3840 x 3840, equisolid, a 190 degree circle, an 8 mm lens, at 8 and at 10 bits.  One call reads 16 x 22
(44) MB and writes 16 x 44 (88) MB, four (eight) times the 256 MB Infinity Cache, so every call finds its frames in HBM whatever ran
before (HBM-cold by size; nothing is flushed between calls).

The time yardstick is the two-pass route on the kernels the library had before this one: gs360_video_rgb on the source, then the
cubic plan remap (gs360_map_plan_create + gs360_remap_plans_u8 / _u16) of the RGB frame with maps taken from the restatement's
coordinates (sx / 32, sy / 32, valid = visible).  Its pixels differ (it converts before it interpolates, and with another cubic) and
are not compared.  Both run in this process, ALTERNATING: `--reps` (>= 5) repetitions of [`--calls` fused calls, `--calls` route
calls], HIP events around each group; the medians and the spread over the repetitions are reported.  Counted bytes per frame (source
planes once, output once) over the fused time are set against the memory-system probe's reading on the same GPU right after
(lib/libgs360probe.so through bench.memsys_probe).  Every 16th row of the device's first view is compared with the restatement's.

    python tests/tools/bench_vidfisheye.py [--reps 5] [--calls 4] [--out profiles/r25/vidfisheye/bench_vidfisheye.json]
    python tests/tools/bench_vidfisheye.py --counters-run          three fused calls per depth and nothing else, for a counter run of its own:
        rocprofv3 --pmc SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_LDS SQ_WAIT_ANY \\
            SQ_WAIT_INST_ANY GRBM_GUI_ACTIVE --output-format csv -d DIR -- python tests/tools/bench_vidfisheye.py --counters-run
    python tests/tools/bench_vidfisheye.py --counters DIR          the shares from that run's counter_collection.csv files
"""
import argparse
import collections
import csv
import glob
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[2]
for p in (str(ROOT), str(ROOT / "360cam-pgm-3dgs-tools_amd"), str(ROOT / "tests")):
    sys.path.insert(0, p)

W = H = S = 3840
N = 16
PROJECTION, INPUT_FOV, FOCAL_MM = "equisolid", 190.0, 8.0


def frames(depth):
    """photo-like planes: smooth fields plus noise, a different phase per frame"""
    rng = np.random.default_rng(depth)
    dt = np.uint8 if depth == 8 else np.uint16
    s = 1 << (depth - 8)
    x = np.arange(W, dtype=np.float32)[None, :]
    y = np.arange(H, dtype=np.float32)[:, None]
    base = 126 + 90 * np.sin(x / 310.0) * np.cos(y / 270.0)
    cbase = 128 + 60 * np.sin(x[:, ::2] / 500.0 + 1.0) * np.cos(y[::2] / 410.0)
    out = []
    for k in range(N):
        Y = np.clip((base + 6 * k + rng.normal(0, 3, base.shape).astype(np.float32)) * s, 16 * s, 235 * s).astype(dt)
        U = np.clip((cbase + 2 * k + rng.normal(0, 2, cbase.shape).astype(np.float32)) * s, 16 * s, 240 * s).astype(dt)
        V = np.clip((256 - cbase - 3 * k) * s, 16 * s, 240 * s).astype(dt)
        out.append((Y, U, V))
    return out


class Workload:
    def __init__(self, ctx, depth, with_route):
        import gs360
        from gs360 import vidfisheye
        import vidfisheye_np as ref
        self.ctx, self.depth = ctx, depth
        self.dtype = np.uint8 if depth == 8 else np.uint16
        item = np.dtype(self.dtype).itemsize
        self.view = vidfisheye.view_from_args(FOCAL_MM, S, PROJECTION, INPUT_FOV)
        self.stage = vidfisheye.FisheyeStage(self.view, depth)
        self.host = frames(depth)
        self.planes = [[ctx.to_device(p) for p in f] for f in self.host]
        self.dsts = [ctx.alloc(S * S * 3 * item) for _ in range(N)]
        self.jobs = [(p[0], p[1], p[2], W, H, "420", d) for p, d in zip(self.planes, self.dsts)]
        self.bufs = [p for f in self.planes for p in f] + self.dsts
        self.plan = None
        if with_route:
            c = ref.coordinates(PROJECTION, S, W, H, self.view.input_fov_deg, self.view.h_fov_deg, self.view.v_fov_deg)
            maps = [ctx.to_device((c[k] / 32.0).astype(np.float32)) for k in ("sx", "sy")] + [ctx.to_device(c["visible"].astype(np.uint8) * 255)]
            self.visible_share = float(c["visible"].mean())
            self.plan = ctx.map_plan(maps[0], maps[1], maps[2], S, S)
            ctx.sync(0)
            for m in maps:
                ctx.free(m)
            self.rgb = [ctx.alloc(H * W * 3 * item) for _ in range(N)]
            self.rgb_jobs = [(p[0], p[1], p[2], W, H, "420", d) for p, d in zip(self.planes, self.rgb)]
            self.remap_jobs = [(r, H, W, self.plan, True, S, S, 0, d) for r, d in zip(self.rgb, self.dsts)]
            self.bufs += self.rgb
            self.gs360 = gs360

    def fused(self):
        self.stage.convert_dev(self.ctx, self.jobs)

    def route(self):
        self.stage.color.convert_dev(self.ctx, self.rgb_jobs)
        self.ctx.remap_plans_dev(self.remap_jobs, 3, interp=self.gs360.INTERP_CUBIC, dtype=self.dtype)

    def timed(self, what, calls):
        self.ctx.event_record(0, 0)
        for _ in range(calls):
            what()
        self.ctx.event_record(0, 1)
        self.ctx.sync(0)
        return self.ctx.event_elapsed_ms(0, 0, 1) / calls

    def close(self):
        if self.plan is not None:
            self.ctx.map_plan_free(self.plan)
        for b in self.bufs:
            self.ctx.free(b)
        self.stage.close()


def bench_depth(ctx, depth, reps, calls):
    import vidfisheye_np as ref
    w = Workload(ctx, depth, with_route=True)
    item = np.dtype(w.dtype).itemsize
    for _ in range(2):
        w.timed(w.fused, 1)
        w.timed(w.route, 1)
    fused, route = [], []
    for _ in range(max(5, reps)):                      # alternating, so that whatever else the host does meets both alike
        fused.append(w.timed(w.fused, calls))
        route.append(w.timed(w.route, calls))
    w.timed(w.fused, 1)                                 # the destinations hold the fused call's views again
    got = ctx.download(w.dsts[0], (S, S, 3), dtype=w.dtype)
    v = w.view
    rows = slice(0, S, 16)                              # every 16th row of the view: the restatement takes a minute for all of them
    want = ref.render(*w.host[0], depth, "420", PROJECTION, S, v.input_fov_deg, v.h_fov_deg, v.v_fov_deg, rows=rows)
    counted = N * (H * W * item * 1.5 + S * S * 3 * item)
    mf, mr = float(np.median(fused)), float(np.median(route))
    res = {"depth": depth, "frames_per_call": N, "source": [W, H], "view": S, "subsampling": "420", "projection": PROJECTION,
           "input_fov_deg": v.input_fov_deg, "h_fov_deg": v.h_fov_deg, "visible_share": w.visible_share,
           "repetitions": len(fused), "calls_per_repetition": calls,
           "fused_ms_per_call": {"median": mf, "min": float(min(fused)), "max": float(max(fused)), "all": [float(x) for x in fused]},
           "route_ms_per_call": {"median": mr, "min": float(min(route)), "max": float(max(route)), "all": [float(x) for x in route]},
           "fused_us_per_frame": 1e3 * mf / N, "route_us_per_frame": 1e3 * mr / N, "fused_over_route": mf / mr,
           "fused_no_slower_within_spread": bool(mf <= mr or min(fused) <= max(route)),
           "counted_bytes_per_frame": counted / N, "counted_gb_per_s": counted / (mf * 1e-3) / 1e9,
           "equals_numpy_restatement_every_16th_row": bool(np.array_equal(got[rows], want))}
    w.close()
    return res


def counters_run():
    import gs360
    with gs360.Context(device=0, n_slots=1) as ctx:
        for depth in (8, 10):
            w = Workload(ctx, depth, with_route=False)
            for _ in range(3):
                w.fused()
            ctx.sync(0)
            w.close()


def counters(directory):
    """per instantiation of vidfisheye_kernel, the means over its launches"""
    acc = collections.defaultdict(lambda: collections.defaultdict(list))
    for f in glob.glob(str(pathlib.Path(directory) / "**" / "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "vidfisheye_kernel" in r["Kernel_Name"]:
                acc["d8" if "<unsigned char>" in r["Kernel_Name"] else "d10"][r["Counter_Name"]].append(float(r["Counter_Value"]))
    out = {}
    for key, c in acc.items():
        m = {n: sum(v) / len(v) for n, v in c.items()}
        cycles = m["GRBM_GUI_ACTIVE"] / 8.0            # summed over the 8 XCDs
        out[key] = {"launches": len(c["GRBM_GUI_ACTIVE"]), "launch_cycles": round(cycles),
                    "valu_busy": round(m["SQ_ACTIVE_INST_VALU"] * 4 / (1024 * cycles), 3),
                    "lds_bank_conflict_share_of_lds_cycles": round(m["SQ_LDS_BANK_CONFLICT"] / m["SQ_LDS_IDX_ACTIVE"], 3),
                    "lds_active_share_of_launch": round(m["SQ_LDS_IDX_ACTIVE"] / (256 * cycles), 3),
                    "wave_cycles_split": {"active": round(m["SQ_ACTIVE_INST_ANY"] / m["SQ_WAVE_CYCLES"], 3) if "SQ_ACTIVE_INST_ANY" in m else None,
                                          "parked": round(m["SQ_WAIT_ANY"] / m["SQ_WAVE_CYCLES"], 3),
                                          "issue_stall": round(m["SQ_WAIT_INST_ANY"] / m["SQ_WAVE_CYCLES"], 3)},
                    "means": {n: round(v) for n, v in sorted(m.items())}}
    return {"formula": "valu_busy = SQ_ACTIVE_INST_VALU x 4 / (1024 SIMDs x GRBM_GUI_ACTIVE / 8); lds_bank_conflict_share = "
                       "SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE; lds_active_share = SQ_LDS_IDX_ACTIVE / (256 CUs x launch cycles)",
            "kernels": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--counters-run", action="store_true")
    ap.add_argument("--counters", default=None)
    a = ap.parse_args()
    if a.counters_run:
        counters_run()
        return
    if a.counters:
        res = counters(a.counters)
    else:
        import gs360
        res = {"command": "python tests/tools/bench_vidfisheye.py --reps {} --calls {}".format(a.reps, a.calls)}
        with gs360.Context(device=0, n_slots=1) as ctx:
            res["device"] = ctx.info()["name"]
            for depth in (8, 10):
                res[f"d{depth}"] = bench_depth(ctx, depth, a.reps, a.calls)
        import bench
        res["memsys_probe_gb_per_s"] = bench.memsys_probe(0)
        if res["memsys_probe_gb_per_s"]:
            top = max(res["memsys_probe_gb_per_s"].values())
            for depth in (8, 10):
                res[f"d{depth}"]["fraction_of_probe_best"] = res[f"d{depth}"]["counted_gb_per_s"] / top
    print(json.dumps(res, sort_keys=True))
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
