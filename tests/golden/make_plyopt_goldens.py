#!/usr/bin/env python3
"""Capture what the unmodified gs360_PlyOptimizer.py computes on small seeded clouds (VOX-SPEC v1).

Runs only in the build container (needs /root/reference).  `plyfile` is not installed there, so the reference module is imported
with an empty stand-in for it in sys.modules; none of the functions called here touches it.  Output is data only: the input clouds,
the voxel sizes, the pick indices and unique counts of the reference's functions, the complete stdout of its two target searches,
its sky points and its colour conversions.

    python tests/golden/make_plyopt_goldens.py     # rewrites plyopt_goldens.npz
"""
import contextlib
import io
import pathlib
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
REF = pathlib.Path("/root/reference")
sys.path.insert(0, str(REF / "cli_tools"))
stub = types.ModuleType("plyfile")
stub.PlyData = stub.PlyElement = object
sys.modules.setdefault("plyfile", stub)

import gs360_PlyOptimizer as ref  # noqa: E402  (reference; container-only)

HERE = pathlib.Path(__file__).resolve().parent
VOXELS = {"mix": [0.25, 0.3, 0.5, 1.0], "long": [0.25, 0.5]}
TARGETS = {"mix": [400, 1500, 3899]}      # the last is above the number of distinct points: the shrink loop runs down to 1e-9
STRATEGIES = ("first", "center", "centroid")


def clouds():
    rng = np.random.default_rng(20261020)
    gauss = rng.normal(size=(3000, 3)) * np.array([4.0, 1.5, 0.5])
    lattice = rng.integers(-8, 9, size=(500, 3)) * 0.25          # points on voxel faces, exact duplicates
    dense = np.array([0.05, 0.05, 0.05]) + rng.uniform(0.0, 0.02, size=(400, 3))   # 400 points inside one voxel
    mix = np.concatenate([gauss, lattice, dense]).astype(np.float32)
    mix = mix[rng.permutation(mix.shape[0])]
    centres = np.stack([rng.uniform(0.0, 3.0e5, 60), rng.uniform(0.0, 2.0, 60), rng.uniform(0.0, 2.0, 60)], axis=1)
    near = centres[rng.integers(0, 60, 1500)] + rng.uniform(-0.4, 0.4, size=(1500, 3))
    far = np.stack([rng.uniform(0.0, 3.0e5, 1000), rng.uniform(0.0, 2.0, 1000), rng.uniform(0.0, 2.0, 1000)], axis=1)
    long = np.concatenate([near, far]).astype(np.float32)        # x keys of 21 bits at voxel 0.25
    long = long[rng.permutation(long.shape[0])]
    return {"mix": mix, "long": long}


def captured(fn, *args, **kw):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = fn(*args, **kw)
    return out, buf.getvalue()


def main():
    out = {}
    for name, xyz in clouds().items():
        rgb = np.random.default_rng(7).integers(0, 256, size=(xyz.shape[0], 3), dtype=np.uint8)
        out[f"{name}/xyz"], out[f"{name}/rgb"] = xyz, rgb
        out[f"{name}/voxels"] = np.array(VOXELS[name], dtype=np.float64)
        stats = ref.compute_point_cloud_stats(xyz)
        out[f"{name}/minmax"] = np.concatenate([stats.xyz_min, stats.xyz_max]).astype(np.float32)
        out[f"{name}/volume"] = np.float64(stats.volume)
        counts = []
        for vi, voxel in enumerate(VOXELS[name]):
            counts.append(ref._unique_voxel_count(xyz, voxel, stats.xyz_min))
            for how in STRATEGIES:
                _x, _c, idx = ref.voxel_downsample_by_size(xyz, rgb, voxel, representative=how, return_indices=True)
                assert idx.shape[0] == counts[-1]
                out[f"{name}/pick/{vi}/{how}"] = idx.astype(np.int64)
        out[f"{name}/counts"] = np.array(counts, dtype=np.int64)
        for target in TARGETS.get(name, []):
            (_x, _c, idx), text = captured(ref.voxel_downsample_to_target, xyz, rgb, target, return_indices=True)
            out[f"{name}/target/{target}/stdout"], out[f"{name}/target/{target}/pick"] = np.array(text), idx.astype(np.int64)
            (_x, _c, idx), text = captured(ref.spatial_hash_downsample_one_pass, xyz, rgb, target_points=target, return_indices=True)
            out[f"{name}/hash/{target}/stdout"], out[f"{name}/hash/{target}/pick"] = np.array(text), idx.astype(np.int64)
    sky = [([0.0, 0.0, 0.0], "+Z", 100.0, 64, [135, 206, 250], 50.0), ([1.5, -2.0, 0.25], "-Y", 10.0, 33, [1, 2, 3], 100.0),
           ([3.0, 4.0, 5.0], "+X", 2.5, 17, [255, 0, 9], 12.5), ([0.5, 0.5, 0.5], "-Z", 7.0, 20, [9, 9, 9], 75.0)]
    out["sky/params"] = np.array([c + [s, n, p] + col for c, _a, s, n, col, p in sky], dtype=np.float64)
    out["sky/axes"] = np.array([a for _c, a, *_r in sky])
    for i, (centre, axis, scale, count, colour, percent) in enumerate(sky):
        pts, cols = ref._generate_sky_points(np.array(centre, np.float32), ref._axis_direction(axis), scale, count,
                                             np.array(colour, np.uint8), sky_percent=percent)
        out[f"sky/{i}/xyz"], out[f"sky/{i}/rgb"] = pts, cols
    rng = np.random.default_rng(3)
    dc = np.concatenate([rng.normal(size=(60, 3)) * 2.0, [[-1.7724539, 1.7724539, 0.0]]]).astype(np.float32)
    out["color/dc"], out["color/dc_rgb"] = dc, ref.convert_3dgs_dc_to_rgb8(dc)
    unit = np.concatenate([rng.uniform(-0.1, 1.0, size=(40, 3)), [[-np.inf, 0.5, 1.0000005]]]).astype(np.float32)
    wide = np.concatenate([rng.uniform(-5.0, 300.0, size=(40, 3)), [[np.inf, 0.5, 254.5]]]).astype(np.float32)
    out["color/unit"], out["color/unit_rgb"] = unit, ref._float_rgb_to_u8(unit)
    out["color/wide"], out["color/wide_rgb"] = wide, ref._float_rgb_to_u8(wide)
    np.savez_compressed(HERE / "plyopt_goldens.npz", **out)
    print("wrote", HERE / "plyopt_goldens.npz", (HERE / "plyopt_goldens.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
