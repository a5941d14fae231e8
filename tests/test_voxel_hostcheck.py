"""The voxel kernels' per-lane arithmetic, checked on the CPU: tests/tools/voxel_hostcheck.hip calls the host-callable functions of
csrc/gs360_voxel.h (the key of a point, a voxel's centre, a lane's pick of a segment) on arrays of their exact size, built with
AddressSanitizer and UndefinedBehaviorSanitizer.  Every case must give the restatement's picks (tests/voxel_np.py) and no
sanitizer report.  A stand-alone program: nothing is loaded into python."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import voxel_cases
import voxel_np
from conftest import GOLDEN, ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
STRATEGIES = {"first": 0, "center": 1, "centroid": 2}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc to build the host check with")
    if os.environ.get("LD_PRELOAD"):
        pytest.skip("a preloaded library and a sanitized program do not go together")
    exe = tmp_path_factory.mktemp("hostcheck") / "voxel_hostcheck"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "tools" / "voxel_hostcheck.hip")],
                   check=True, capture_output=True, timeout=600)
    return exe


def check(program, tmp_path, xyz, voxel, minmax=None, bad=0):
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    true_minmax = voxel_np.bounds(xyz)
    minmax = true_minmax if minmax is None else minmax
    bits = voxel_np.layout(minmax, voxel)
    kmax = voxel_np.axis_keys(minmax[3:].reshape(1, 3), minmax[:3], voxel)[0].astype(np.uint64)
    for how, code in STRATEGIES.items():
        head = struct.pack("<q4i", xyz.shape[0], code, bits[1] + bits[2], bits[2], 0)
        (tmp_path / "in.bin").write_bytes(head + np.append(minmax[:3], np.float32(voxel)).astype("<f4").tobytes() + kmax.astype("<u8").tobytes() +
                                          xyz.tobytes())
        r = subprocess.run([str(program), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (how, r.stderr[-3000:])
        k, outside = (int(v) for v in r.stdout.split())
        assert (outside > 0) == (bad > 0)
        if not bad:
            want = voxel_np.pick(xyz, voxel, how, minmax)
            assert k == want.shape[0] and np.array_equal(np.fromfile(tmp_path / "out.bin", np.uint32), want), (voxel, how)


def test_golden_clouds(program, tmp_path):
    gold = np.load(GOLDEN / "plyopt_goldens.npz")
    for name in ("mix", "long"):
        for voxel in gold[f"{name}/voxels"]:
            check(program, tmp_path, gold[f"{name}/xyz"], float(voxel))


def test_layout_edges(program, tmp_path):
    rng = np.random.default_rng(64)
    check(program, tmp_path, [[1.5, -2.0, 3.25]], 0.5)                                         # one point, no key bits at all
    top = np.array([(1 << 22) - 1, (1 << 21) - 1, (1 << 21) - 1])
    pts = np.concatenate([np.stack([rng.integers(0, t + 1, 200) for t in top], axis=1), [top], [[0, 0, 0]]])
    check(program, tmp_path, np.concatenate([pts, pts[:50]]), 1.0)                             # 22 + 21 + 21 = 64 bits
    flat = np.concatenate([np.stack([np.zeros(200), rng.integers(0, 1 << 24, 200), rng.integers(0, 1 << 24, 200)], axis=1),
                           [[0, (1 << 24) - 1, (1 << 24) - 1], [0, 0, 0]]])
    check(program, tmp_path, flat, 1.0)                                                        # no x bits: shift 48
    cube = np.concatenate([rng.uniform(0.0, 1.0, size=(100, 3)), [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]])
    check(program, tmp_path, cube, 1.0)                                                        # the maximum on the upper face


@pytest.mark.parametrize("bits", voxel_cases.PACKED_LAYOUTS, ids=lambda b: "+".join(map(str, b)))
def test_packed_layouts_up_to_64_bits(program, tmp_path, bits):
    """the lattices of tests/test_voxel_edges_gpu.py; from 0 + 32 + 32 on the x keys' shift is 64, which vx_point_key and vx_center
    must not carry out"""
    xyz = voxel_cases.lattice(bits)
    assert voxel_np.layout(voxel_np.bounds(xyz), 1.0) == list(bits)
    check(program, tmp_path, xyz, 1.0)


def test_squared_distances_at_the_edges_of_float32(program, tmp_path):
    """subnormal squares are told apart; among infinite ones a lane keeps its first point"""
    xyz, members = voxel_cases.subnormal_cloud(23, seed=23)
    assert voxel_np.pick(xyz, 1.0, "centroid")[0] not in (members[0], members[-1])
    check(program, tmp_path, xyz, 1.0)
    xyz, corner, _mixed = voxel_cases.overflow_cloud(20, seed=20)
    assert voxel_np.pick(xyz, 1e20, "center")[0] == voxel_np.pick(xyz, 1e20, "centroid")[0] == corner[0]
    check(program, tmp_path, xyz, 1e20)


def test_points_outside_the_bounds_are_counted_not_read_past(program, tmp_path):
    gold = np.load(GOLDEN / "plyopt_goldens.npz")
    xyz = gold["mix/xyz"][:300]
    minmax = voxel_np.bounds(xyz)
    minmax[3:] = minmax[:3] + np.float32(0.5) * (minmax[3:] - minmax[:3])
    check(program, tmp_path, xyz, 0.25, minmax=minmax, bad=1)
    broken = xyz.copy()
    broken[7, 2] = np.nan
    check(program, tmp_path, broken, 0.25, minmax=voxel_np.bounds(xyz), bad=1)
