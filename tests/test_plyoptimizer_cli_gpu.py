"""gs360_PlyOptimizer.py on the device: -v and -t runs with an appended file and a sky dome on a 20 000-point PLY.  The output bytes
equal the file built from the NumPy restatement's picks (tests/voxel_np.py), the log equals the search driven by its counts."""
import contextlib
import io
import re

import numpy as np
import pytest

import gs360_PlyOptimizer as tool
import voxel_np
from gs360 import pointcloud

pytestmark = pytest.mark.gpu


class HostCloud:
    """what gs360.pointcloud.Cloud offers, computed by the restatement"""

    def __init__(self, xyz):
        self.xyz, self.n, self.minmax = xyz, xyz.shape[0], voxel_np.bounds(xyz)

    def stats(self):
        return pointcloud.compute_point_cloud_stats(self.xyz)

    def unique_count(self, voxel):
        return voxel_np.unique_count(self.xyz, float(voxel), self.minmax)[0]

    def downsample_by_size(self, voxel, representative="centroid", return_indices=True):
        return voxel_np.pick(self.xyz, float(voxel), representative, self.minmax)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    root = tmp_path_factory.mktemp("plyopt")
    rng = np.random.default_rng(20000)
    shell = rng.normal(size=(20000, 3))
    shell = shell / np.linalg.norm(shell, axis=1, keepdims=True) * np.array([6.0, 4.0, 1.5]) + rng.normal(size=(20000, 3)) * 0.03
    xyz, rgb = shell.astype(np.float32), rng.integers(0, 256, size=(20000, 3), dtype=np.uint8)
    pointcloud.save_ply_binary_little(str(root / "cloud.ply"), xyz, rgb)
    extra_xyz, extra_rgb = (rng.uniform(-1, 1, size=(37, 3)) + [20.0, 0.0, 0.0]).astype(np.float32), rng.integers(0, 256, size=(37, 3), dtype=np.uint8)
    pointcloud.save_ply_binary_little(str(root / "extra.ply"), extra_xyz, extra_rgb)
    return root, xyz, rgb, extra_xyz, extra_rgb


def expected_file(xyz, rgb, idx, extra_xyz, extra_rgb, sky_count):
    xyz, rgb = np.concatenate([xyz[idx], extra_xyz]), np.concatenate([rgb[idx], extra_rgb])
    centre = ((xyz.min(axis=0) + xyz.max(axis=0)) * np.float32(0.5)).astype(np.float32)
    sky, cols = pointcloud._generate_sky_points(centre, pointcloud._axis_direction("+Z"), 100.0, sky_count, np.array([135, 206, 250], np.uint8))
    return pointcloud.ply_binary_little_bytes(np.concatenate([xyz, sky]), np.concatenate([rgb, cols]))


def run(argv, capsys):
    assert tool.main(argv) == 0
    return capsys.readouterr().out.splitlines()


@pytest.mark.parametrize("how", ["centroid", "center", "first"])
def test_fixed_voxel_size(scene, capsys, how):
    root, xyz, rgb, extra_xyz, extra_rgb = scene
    out = root / f"v_{how}.ply"
    lines = run(["-i", str(root / "cloud.ply"), "-o", str(out), "-v", "0.35", "-k", how, "-a", "extra.ply", "--sky-axis", "+Z", "--sky-count", "50"], capsys)
    idx = voxel_np.pick(xyz, 0.35, how)
    k = idx.shape[0]
    assert out.read_bytes() == expected_file(xyz, rgb, idx, extra_xyz, extra_rgb, 50)
    assert lines[0] == f"[load] kind=ply base={root / 'cloud.ply'}  points=20,000" and lines[1] == "input_points=20,000"
    assert re.fullmatch(r"\[aabb\] min=\(.+\)  max=\(.+\)  extent=\(.+\)  volume~\S+", lines[2]) and lines[3].startswith("[init] v0~")
    assert lines[4:] == ["[downsample] fixed voxel-size=0.35", f"[downsample] -> {k:,} points", f"[append] {root / 'extra.ply'} +37 -> total {k + 37:,}",
                         "[append] total added: 37", f"[sky] axis=+Z scale=100 percent=50 count=50 -> total {k + 87:,}",
                         f"[save] {out}  points={k + 87:,}  (binary little-endian PLY)"]


@pytest.mark.parametrize("method", ["voxel", "spatial-hash"])
def test_target_points(scene, capsys, method):
    root, xyz, rgb, extra_xyz, extra_rgb = scene
    out = root / f"t_{method}.ply"
    lines = run(["-i", str(root / "cloud.ply"), "-o", str(out), "-t", "2000", "--downsample-method", method, "-a", str(root / "extra.ply"),
                 "--sky-axis", "+Z", "--sky-count", "50"], capsys)
    stats = pointcloud.compute_point_cloud_stats(xyz)
    text = io.StringIO()
    with contextlib.redirect_stdout(text):                  # the same search arithmetic over the restatement's counts and picks
        if method == "voxel":
            want = pointcloud.voxel_downsample_to_target(xyz, rgb, 2000, stats=stats, log_bounds=False, return_indices=True, cloud=HostCloud(xyz))
        else:
            want = pointcloud.spatial_hash_downsample_one_pass(xyz, rgb, target_points=2000, stats=stats, return_indices=True, cloud=HostCloud(xyz))
    k = want[2].shape[0]
    assert abs(k - 2000) <= (40 if method == "voxel" else 400)
    assert out.read_bytes() == expected_file(xyz, rgb, want[2], extra_xyz, extra_rgb, 50)
    assert lines[:3] == [f"[load] kind=ply base={root / 'cloud.ply'}  points=20,000", "input_points=20,000", lines[2]] and lines[2].startswith("[aabb] min=(")
    search = text.getvalue().splitlines()
    assert lines[3:3 + len(search)] == search
    tail = lines[3 + len(search):]
    if method == "voxel":
        assert search[0] == "[target] input_points=20,000  target=2,000  tol=+/-2.0%  max_iter=32" and search[1].startswith("[init] v0~")
        assert all(re.fullmatch(r"\[expand\] try hi=\S+ -> unique=[\d,]+|\[iter \d\d\] voxel=\d+\.\d\d  unique=[\d,]+", ln) for ln in search[2:-3])
        assert re.fullmatch(r"\[stop\] within tolerance: voxel=\S+  unique=[\d,]+", search[-3]) and search[-2].startswith("[best] voxel~")
        assert search[-1] == f"[final] voxel={search[-3].split('voxel=')[1].split()[0]}  out_points={k:,}"
        assert tail[0] == f"[downsample] target_points=2,000 -> {k:,} points"
        tail = tail[1:]
    else:
        assert re.fullmatch(r"\[spatial-hash probe 1\] voxel=\S+ unique=[\d,]+", search[0]) and search[-1].endswith(f"out_points={k:,} (approx)")
    assert tail == [f"[append] {root / 'extra.ply'} +37 -> total {k + 37:,}", "[append] total added: 37",
                    f"[sky] axis=+Z scale=100 percent=50 count=50 -> total {k + 87:,}", f"[save] {out}  points={k + 87:,}  (binary little-endian PLY)"]


def test_random_keeps_one_point_per_voxel(scene, capsys):
    root, xyz, _rgb, _ex, _ec = scene
    out = root / "random.ply"
    lines = run(["-i", str(root / "cloud.ply"), "-o", str(out), "-v", "0.35", "-k", "random"], capsys)
    got, _cols = pointcloud.load_ply_xyz_rgb(str(out))
    minmax = voxel_np.bounds(xyz)
    assert np.array_equal(voxel_np.packed_keys(got, minmax, 0.35), np.unique(voxel_np.packed_keys(xyz, minmax, 0.35)))
    assert lines[-1] == f"[save] {out}  points={got.shape[0]:,}  (binary little-endian PLY)"
