"""OCT-SPEC v1 without a GPU: the NumPy restatement (tests/octree_np.py) gives the unmodified reference's index arrays
(tests/golden/octree_goldens.npz) on the whole grid, the module function's exits that need no device, and the CLI's gated path on a
machine without one."""
import numpy as np
import pytest

import gs360_PlyOptimizer as tool
import octree_cases
import octree_np
from conftest import GOLDEN
from gs360 import capi, pointcloud


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN / "octree_goldens.npz")


def test_restatement_equals_the_reference_on_the_grid(gold):
    xyz = gold["mix/xyz"]
    assert xyz.shape == (2300, 3) and len(gold["mix/targets"]) * len(gold["mix/weights"]) * len(gold["mix/min_voxels"]) * 3 == 270
    for ti, target in enumerate(gold["mix/targets"]):
        for wi, weight in enumerate(gold["mix/weights"]):
            for vi, min_voxel in enumerate(gold["mix/min_voxels"]):
                for how in octree_cases.STRATEGIES:
                    got = octree_np.pick(xyz, int(target), float(weight), float(min_voxel) or None, how)
                    assert np.array_equal(got, gold[f"mix/pick/{ti}/{wi}/{vi}/{how}"]), (target, weight, min_voxel, how)


def test_restatement_equals_the_reference_on_leaves_of_tens_of_thousands(gold):
    xyz = gold["big/xyz"]
    for ti, target in enumerate(gold["big/targets"]):
        sizes = [idx.shape[0] for idx, _d in octree_np.segments(xyz, int(target))[0]]
        assert max(sizes) == 70000 if target == 1 else max(sizes) > 10000
        for how in octree_cases.STRATEGIES:
            assert np.array_equal(octree_np.pick(xyz, int(target), how=how), gold[f"big/pick/{ti}/{how}"]), (target, how)


def test_edge_clouds_are_what_they_claim():
    by_name = {name: (xyz, runs) for name, xyz, runs in octree_cases.cases()}
    xyz, _runs = by_name["centre planes"]
    cube_min, cube_size = octree_np.cube(xyz)
    assert np.array_equal(cube_min, [0, 0, 0]) and cube_size == 64.0
    code = octree_np.codes(xyz, cube_min, cube_size)
    assert code.max() == (1 << 36) - 1 and code.min() == 0
    xyz, _runs = by_name["leaf lengths around 32 and 64"]
    assert sorted(idx.shape[0] for idx, _d in octree_np.segments(xyz, 6)[0]) == [31, 32, 33, 63, 64, 65]
    xyz, _runs = by_name["identical points"]
    assert octree_np.cube(xyz)[1] == float(np.float32(1e-9)) and octree_np.pick(xyz, 5).tolist() == [0]
    xyz, _runs = by_name["five-fold duplicates"]
    assert {d for _i, d in octree_np.segments(xyz, 149)[0]} >= {12} and octree_np.pick(xyz, 149).shape[0] == 30
    xyz, _runs = by_name["all distances tied"]
    assert octree_np.pick(xyz, 1, how="centroid").tolist() == octree_np.pick(xyz, 1, how="center").tolist() == [0]


def test_exits_that_need_no_device():
    xyz = np.arange(15, dtype=np.float64).reshape(5, 3)
    rgb = np.arange(15, dtype=np.int64).reshape(5, 3)
    for target in (None, 0, -3, 5, 9):
        out = pointcloud.adaptive_voxel_downsample(xyz, rgb, target, return_indices=True, max_depth=3)
        assert out[0].dtype == np.float32 and out[1].dtype == np.uint8 and np.array_equal(out[0], xyz) and np.array_equal(out[1], rgb)
        assert out[2].dtype == np.int64 and np.array_equal(out[2], np.arange(5))
    assert len(pointcloud.adaptive_voxel_downsample(xyz, rgb, 5)) == 2
    out = pointcloud.adaptive_voxel_downsample(xyz[:0], rgb[:0], 3, return_indices=True)
    assert out[0].shape == (0, 3) and out[2].shape == (0,) and out[2].dtype == np.int64
    with pytest.raises(capi.Gs360Error) as e:
        pointcloud.adaptive_voxel_downsample(xyz, rgb, 2, max_depth=8)
    assert e.value.code == capi.ERR_UNSUPPORTED


def test_the_gate_is_off_by_default_and_says_what_it_takes(monkeypatch):
    monkeypatch.delenv("GS360_PLY_ADAPTIVE", raising=False)
    assert pointcloud.adaptive_mode_from_env() is False
    monkeypatch.setenv("GS360_PLY_ADAPTIVE", "device")
    assert pointcloud.adaptive_mode_from_env() is True
    monkeypatch.setenv("GS360_PLY_ADAPTIVE", "host")
    with pytest.raises(ValueError):
        pointcloud.adaptive_mode_from_env()


@pytest.mark.parametrize("extra", [["--adaptive", "-t", "2"], ["--downsample-method", "adaptive", "-r", "50", "-v", "0.5"]])
def test_gated_run_without_a_gpu_is_one_error_line(tmp_path, capsys, monkeypatch, extra):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here")
    monkeypatch.setenv("GS360_PLY_ADAPTIVE", "device")
    xyz = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 4.0], [0.5, 1.0, 1.0], [1.0, 0.0, 0.0]], dtype=np.float32)
    pointcloud.save_ply_binary_little(str(tmp_path / "cloud.ply"), xyz, np.zeros((4, 3), np.uint8))
    out = tmp_path / "out.ply"
    assert tool.main(["-i", str(tmp_path / "cloud.ply"), "-o", str(out)] + extra) == 1
    lines = capsys.readouterr().out.splitlines()
    errs = [ln for ln in lines if ln.startswith("[ERR]")]
    assert len(errs) == 1 and "gs360 error -3" in errs[0] and lines[-1] == errs[0]
    assert any(ln.startswith("[adaptive] weight=1 min_voxel=") for ln in lines)
    assert not out.exists()


def test_gated_run_that_keeps_every_point_needs_no_gpu(tmp_path, capsys, monkeypatch):
    """no target: the reference's own pass-through (PLY:1217-1222), with its lines"""
    monkeypatch.setenv("GS360_PLY_ADAPTIVE", "device")
    xyz = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 4.0], [0.5, 1.0, 1.0]], dtype=np.float32)
    rgb = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], dtype=np.uint8)
    pointcloud.save_ply_binary_little(str(tmp_path / "cloud.ply"), xyz, rgb)
    out = tmp_path / "out.ply"
    assert tool.main(["-i", str(tmp_path / "cloud.ply"), "-o", str(out), "--adaptive", "--adaptive-weight", "0.25"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines[4:] == ["[warn] --adaptive is deprecated by --downsample-method; forcing method=adaptive.",
                         "[adaptive] target not specified; defaulting to input count (no reduction).", "[adaptive] weight=0.25 min_voxel=auto",
                         "[adaptive] target~3 -> 3 points", f"[save] {out}  points=3  (binary little-endian PLY)"]
    assert out.read_bytes() == pointcloud.ply_binary_little_bytes(xyz, rgb)
