#!/usr/bin/env python3
"""Capture what the unmodified gs360_PlyOptimizer.py's adaptive_voxel_downsample returns on seeded clouds (OCT-SPEC v1).

Runs only in the build container (needs /root/reference).  `plyfile` is not installed there, so the reference module is imported
with an empty stand-in for it in sys.modules; the three CLI runs get their cloud from, and hand their result to, two functions put
in place of the reference's PLY reader and writer (the only users of `plyfile`).  Output is data only: the input clouds, the grid of
parameters, the index arrays, the CLI's stdout (its folder written as {dir}) and the points and colours it would have saved.

    python tests/golden/make_octree_goldens.py     # rewrites octree_goldens.npz
"""
import contextlib
import io
import pathlib
import sys
import tempfile
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
STRATEGIES = ("centroid", "center", "first")
WEIGHTS = (1.0, 0.0, 0.5, 2.0, -1.0)
MIN_VOXELS = (0.0, 0.75)                  # 0: none
BIG_TARGETS = (1, 2, 9)
CLI_RUNS = (["--adaptive", "-t", "300"], ["--downsample-method", "adaptive", "-r", "12.5", "-v", "0.4", "--adaptive-weight", "0.5"],
            ["--downsample-method", "adaptive", "-t", "64", "-k", "first"])


def clouds():
    rng = np.random.default_rng(20261021)
    gauss = rng.normal(size=(1500, 3)) * np.array([4.0, 1.5, 0.5])
    dup = np.repeat(rng.normal(size=(40, 3)) * 2.0, 5, axis=0)                       # 40 points, five times each: depth 12 with count 5
    lattice = rng.integers(-8, 9, size=(400, 3)) * 0.25
    dense = np.array([0.05, 0.05, 0.05]) + rng.uniform(0.0, 0.02, size=(200, 3))
    mix = np.concatenate([gauss, dup, lattice, dense]).astype(np.float32)
    mix = mix[rng.permutation(mix.shape[0])]
    big = np.rint(rng.normal(size=(70000, 3)) * np.array([8.0, 3.0, 1.0]) * 16.0) / 16.0   # sixteenths: small when compressed
    return {"mix": mix, "big": big.astype(np.float32)}


def indices(xyz, rgb, target, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return ref.adaptive_voxel_downsample(xyz, rgb, target, return_indices=True, **kw)[2].astype(np.int32)


def main():
    out = {}
    both = clouds()
    for name, xyz in both.items():
        out[f"{name}/xyz"] = xyz
    mix, big = both["mix"], both["big"]
    n = mix.shape[0]
    rgb = np.random.default_rng(7).integers(0, 256, size=(n, 3), dtype=np.uint8)
    out["mix/rgb"] = rgb
    targets = (1, 2, 7, 8, 9, 50, 230, 1000, n - 1)
    out["mix/targets"], out["mix/weights"], out["mix/min_voxels"] = np.array(targets), np.array(WEIGHTS), np.array(MIN_VOXELS)
    out["big/targets"] = np.array(BIG_TARGETS)
    for ti, target in enumerate(targets):
        for wi, weight in enumerate(WEIGHTS):
            for vi, min_voxel in enumerate(MIN_VOXELS):
                for how in STRATEGIES:
                    out[f"mix/pick/{ti}/{wi}/{vi}/{how}"] = indices(mix, rgb, target, weight_power=weight, min_voxel_size=min_voxel or None,
                                                                    representative=how)
    big_rgb = np.zeros((big.shape[0], 3), dtype=np.uint8)
    for ti, target in enumerate(BIG_TARGETS):
        for how in STRATEGIES:
            out[f"big/pick/{ti}/{how}"] = indices(big, big_rgb, target, representative=how)
    saved = {}
    ref.load_ply_xyz_rgb = lambda path: (mix, rgb)
    ref.save_ply_binary_little = lambda path, xyz, rgb: saved.update(xyz=xyz, rgb=rgb)
    with tempfile.TemporaryDirectory() as tmp:
        tmp = str(pathlib.Path(tmp).resolve())
        for ri, argv in enumerate(CLI_RUNS):
            text = io.StringIO()
            with contextlib.redirect_stdout(text):
                assert ref.main(["-i", f"{tmp}/cloud.ply", "-o", f"{tmp}/out.ply"] + argv) == 0
            out[f"cli/{ri}/argv"], out[f"cli/{ri}/stdout"] = np.array(argv), np.array(text.getvalue().replace(tmp, "{dir}"))
            out[f"cli/{ri}/xyz"], out[f"cli/{ri}/rgb"] = saved["xyz"].astype(np.float32), saved["rgb"].astype(np.uint8)
    np.savez_compressed(HERE / "octree_goldens.npz", **out)
    print("wrote", HERE / "octree_goldens.npz", (HERE / "octree_goldens.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
