"""The octree sampling's host-callable steps, checked on the CPU: tests/tools/octree_hostcheck.hip calls csrc/gs360_octree.h's
functions (the path code of a point, the divergence level of two codes, the split loop over counts, a lane's pick of a leaf, the
selection) on arrays of their exact size, built with AddressSanitizer and UndefinedBehaviorSanitizer.  Every case must give the
reference's picks (tests/golden/octree_goldens.npz) or the restatement's (tests/octree_np.py), and no sanitizer report.  A
stand-alone program: nothing is loaded into python."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import octree_cases
import octree_np
from conftest import GOLDEN, ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
STRATEGIES = {"first": 0, "center": 1, "centroid": 2}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc to build the host check with")
    if os.environ.get("LD_PRELOAD"):
        pytest.skip("a preloaded library and a sanitized program do not go together")
    exe = tmp_path_factory.mktemp("hostcheck") / "octree_hostcheck"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "tools" / "octree_hostcheck.hip")],
                   check=True, capture_output=True, timeout=600)
    return exe


def run(program, tmp_path, xyz, target, power, min_voxel, how):
    """-> (picks, number of leaves, largest code)"""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    cube_min, cube_size = octree_np.cube(xyz)
    head = struct.pack("<2q2i3d", xyz.shape[0], target, STRATEGIES[how], 0, power, min_voxel or 0.0, cube_size)
    (tmp_path / "in.bin").write_bytes(head + np.append(cube_min, np.float32(0)).astype("<f4").tobytes() + xyz.tobytes())
    r = subprocess.run([str(program), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (how, r.stderr[-3000:])
    k, leaves, top = r.stdout.split()
    picks = np.fromfile(tmp_path / "out.bin", np.uint32)
    assert picks.shape[0] == int(k)
    return picks, int(leaves), int(top, 16)


def test_golden_grid(program, tmp_path):
    """every third case of the reference's grid (each strategy, target, weight and smallest voxel several times)"""
    gold = np.load(GOLDEN / "octree_goldens.npz")
    xyz, at = gold["mix/xyz"], 0
    for ti, target in enumerate(gold["mix/targets"]):
        for wi, weight in enumerate(gold["mix/weights"]):
            for vi, min_voxel in enumerate(gold["mix/min_voxels"]):
                for hi, how in enumerate(octree_cases.STRATEGIES):
                    at += 1
                    if (at + hi) % 3:
                        continue
                    picks, _leaves, _top = run(program, tmp_path, xyz, int(target), float(weight), float(min_voxel), how)
                    assert np.array_equal(picks, gold[f"mix/pick/{ti}/{wi}/{vi}/{how}"]), (target, weight, min_voxel, how)


def test_leaves_of_tens_of_thousands(program, tmp_path):
    """the float32 centroid sum, point by point, is what pts.mean(axis=0) gave the reference"""
    gold = np.load(GOLDEN / "octree_goldens.npz")
    for ti, target in enumerate(gold["big/targets"]):
        for how in octree_cases.STRATEGIES:
            picks, _leaves, _top = run(program, tmp_path, gold["big/xyz"], int(target), 1.0, None, how)
            assert np.array_equal(picks, gold[f"big/pick/{ti}/{how}"]), (target, how)


@pytest.mark.parametrize("case", octree_cases.cases(), ids=lambda c: c[0])
def test_edge_clouds(program, tmp_path, case):
    name, xyz, runs = case
    for target, power, min_voxel in runs:
        for how in octree_cases.STRATEGIES:
            picks, leaves, top = run(program, tmp_path, xyz, target, power, min_voxel, how)
            assert np.array_equal(picks, octree_np.pick(xyz, target, power, min_voxel, how)), (name, target, power, min_voxel, how)
            assert picks.shape[0] <= target <= max(leaves, target) and leaves < xyz.shape[0] + 8
            if name == "centre planes":
                assert top == (1 << 36) - 1
