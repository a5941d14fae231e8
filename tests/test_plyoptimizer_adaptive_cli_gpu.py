"""gs360_PlyOptimizer.py --downsample-method adaptive on the device, with GS360_PLY_ADAPTIVE=device: the three recorded runs of the
unmodified reference (tests/golden/octree_goldens.npz) -- its stdout line for line and the bytes of the PLY it would have saved."""
import numpy as np
import pytest

import gs360_PlyOptimizer as tool
from conftest import GOLDEN
from gs360 import pointcloud

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("run", [0, 1, 2], ids=["--adaptive -t", "-r -v --adaptive-weight", "-k first"])
def test_recorded_runs(tmp_path, capsys, monkeypatch, run):
    gold = np.load(GOLDEN / "octree_goldens.npz")
    monkeypatch.setenv("GS360_PLY_ADAPTIVE", "device")
    tmp_path = tmp_path.resolve()
    pointcloud.save_ply_binary_little(str(tmp_path / "cloud.ply"), gold["mix/xyz"], gold["mix/rgb"])
    argv = [str(a) for a in gold[f"cli/{run}/argv"]]
    assert all(flag in argv for flag in [("--adaptive", "-t"), ("--downsample-method", "adaptive", "-r", "-v"), ("adaptive", "-k", "first")][run])
    assert tool.main(["-i", str(tmp_path / "cloud.ply"), "-o", str(tmp_path / "out.ply")] + argv) == 0
    assert capsys.readouterr().out == str(gold[f"cli/{run}/stdout"]).replace("{dir}", str(tmp_path))
    assert (tmp_path / "out.ply").read_bytes() == pointcloud.ply_binary_little_bytes(gold[f"cli/{run}/xyz"], gold[f"cli/{run}/rgb"])


def test_without_the_variable_the_flag_is_still_refused(tmp_path, capsys, monkeypatch):
    monkeypatch.delenv("GS360_PLY_ADAPTIVE", raising=False)
    gold = np.load(GOLDEN / "octree_goldens.npz")
    pointcloud.save_ply_binary_little(str(tmp_path / "cloud.ply"), gold["mix/xyz"], gold["mix/rgb"])
    assert tool.main(["-i", str(tmp_path / "cloud.ply"), "-o", str(tmp_path / "out.ply"), "--adaptive", "-t", "300"]) == 1
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 1 and lines[0].startswith("[ERR] ") and not (tmp_path / "out.ply").exists()
