"""VOX-SPEC v1 on the CPU: the NumPy restatement (tests/voxel_np.py) against what the reference recorded
(tests/golden/plyopt_goldens.npz), the key layout at the 64-bit boundary, the host path of gs360/pointcloud.py, its PLY reader and
writer, its sky points and colour conversions."""
import re
import struct

import numpy as np
import pytest

import voxel_cases
import voxel_np
from conftest import GOLDEN, PKG
from gs360 import pointcloud

CLOUDS = ("mix", "long")
STRATEGIES = ("first", "center", "centroid")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN / "plyopt_goldens.npz")


def cases(gold):
    for name in CLOUDS:
        for vi, voxel in enumerate(gold[f"{name}/voxels"]):
            yield name, vi, float(voxel)


def test_golden_clouds_hold_what_the_spec_needs(gold):
    mix, long = gold["mix/xyz"], gold["long/xyz"]
    assert mix.dtype == long.dtype == np.float32
    assert np.unique(mix, axis=0).shape[0] < mix.shape[0]                        # exact duplicates
    assert np.count_nonzero(np.all(mix * 4 == np.round(mix * 4), axis=1)) >= 500   # points on voxel faces
    for voxel in gold["mix/voxels"]:                                            # one crowded voxel
        keys = voxel_np.triple_keys(mix, voxel_np.bounds(mix), float(voxel))
        assert np.unique(keys, axis=0, return_counts=True)[1].max() >= 400
    assert voxel_np.layout(voxel_np.bounds(long), 0.25)[0] >= 20


def test_restatement_equals_the_reference(gold):
    for name, vi, voxel in cases(gold):
        xyz = gold[f"{name}/xyz"]
        assert np.array_equal(voxel_np.bounds(xyz), gold[f"{name}/minmax"])
        count, packed = voxel_np.unique_count(xyz, voxel)
        assert packed and count == gold[f"{name}/counts"][vi], (name, voxel)
        for how in STRATEGIES:
            assert np.array_equal(voxel_np.pick(xyz, voxel, how), gold[f"{name}/pick/{vi}/{how}"]), (name, voxel, how)


def test_host_path_equals_the_reference(gold):
    """what gs360/pointcloud.py computes where the device refuses a grid"""
    for name, vi, voxel in cases(gold):
        xyz, lo = gold[f"{name}/xyz"], gold[f"{name}/minmax"][:3]
        assert pointcloud._host_unique_count(xyz, voxel, lo) == gold[f"{name}/counts"][vi]
        for how in STRATEGIES:
            assert np.array_equal(pointcloud._host_pick(xyz, voxel, lo, how), gold[f"{name}/pick/{vi}/{how}"]), (name, voxel, how)


def test_stats_equal_the_reference(gold):
    for name in CLOUDS:
        stats = pointcloud.compute_point_cloud_stats(gold[f"{name}/xyz"])
        assert np.array_equal(np.concatenate([stats.xyz_min, stats.xyz_max]), gold[f"{name}/minmax"])
        assert stats.volume == float(gold[f"{name}/volume"]) and stats.extent.dtype == np.float32


def lattice_cloud(bits, seed):
    """integer coordinates (voxel 1.0) whose largest keys have exactly `bits` bits per axis; duplicates included"""
    rng = np.random.default_rng(seed)
    top = np.array([(1 << b) - 1 for b in bits], dtype=np.int64)
    pts = np.stack([rng.integers(0, t + 1, 300) for t in top], axis=1)
    pts = np.concatenate([pts, pts[:40], [top], [[0, 0, 0]]])
    return pts.astype(np.float32)                          # every coordinate is below 2^24: exact


@pytest.mark.parametrize("bits,packed", [((22, 21, 21), True), ((23, 21, 21), False), ((0, 24, 24), True), ((21, 22, 22), False)])
def test_key_layout_around_64_bits(bits, packed):
    xyz = lattice_cloud(bits, sum(bits))
    minmax = voxel_np.bounds(xyz)
    assert (voxel_np.layout(minmax, 1.0) is not None) == packed
    if packed:
        assert voxel_np.layout(minmax, 1.0) == list(bits)
    count, took_packed = voxel_np.unique_count(xyz, 1.0)
    assert took_packed == packed
    distinct = np.unique(xyz, axis=0).shape[0]
    assert count == distinct == np.unique(voxel_np.triple_keys(xyz, minmax, 1.0), axis=0).shape[0]
    assert pointcloud._host_unique_count(xyz, 1.0, minmax[:3]) == distinct


def test_the_cases_know_the_kernels_constants():
    """tests/voxel_cases.py sizes its clouds by the tile, scan and bounds constants of csrc/gs360_voxel.h and the lane threshold of
    csrc/gs360_cloudsteps.h"""
    text = (PKG / "csrc" / "gs360_voxel.h").read_text() + (PKG / "csrc" / "gs360_cloudsteps.h").read_text()
    value = lambda name: int(re.search(rf"constexpr int {name} = (\d+);", text).group(1))
    got = (voxel_cases.TILE, voxel_cases.SCAN_THREADS, voxel_cases.BOUND_BLOCKS, voxel_cases.BOUND_THREADS, voxel_cases.LANE_MAX)
    assert got == tuple(value(n) for n in ("kVxTile", "kVxScanThreads", "kVxBoundBlocks", "kVxThreads", "kCloudLaneMax"))


def test_a_grid_of_1e9_per_unit_takes_the_host_path(gold):
    xyz = gold["mix/xyz"]
    count, packed = voxel_np.unique_count(xyz, 1e-9)
    assert not packed and count == np.unique(xyz, axis=0).shape[0]


# ---- PLY ----------------------------------------------------------------------------------------------------------------------------
XYZ = np.array([[0.0, 1.5, -2.25], [3.0, 4.0, 5.0], [1e-3, -1e6, 7.0]], dtype=np.float32)
RGB = np.array([[0, 128, 255], [1, 2, 3], [250, 9, 77]], dtype=np.uint8)
HEADER = (b"ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
          b"property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")


def test_writer_bytes(tmp_path):
    want = HEADER + b"".join(struct.pack("<fffBBB", *[float(v) for v in p], *[int(c) for c in col]) for p, col in zip(XYZ, RGB))
    assert pointcloud.ply_binary_little_bytes(XYZ, RGB) == want
    pointcloud.save_ply_binary_little(str(tmp_path / "a.ply"), XYZ.astype(np.float64), RGB.astype(np.int32))
    assert (tmp_path / "a.ply").read_bytes() == want
    with pytest.raises(ValueError):
        pointcloud.ply_binary_little_bytes(XYZ, RGB[:2])


def test_reader_round_trips(tmp_path):
    path = tmp_path / "le.ply"
    path.write_bytes(pointcloud.ply_binary_little_bytes(XYZ, RGB))
    xyz, rgb = pointcloud.load_ply_xyz_rgb(str(path))
    assert xyz.dtype == np.float32 and rgb.dtype == np.uint8
    assert np.array_equal(xyz, XYZ) and np.array_equal(rgb, RGB)
    # big-endian, double coordinates, a normal between position and colour, a face element behind the vertices
    head = (b"ply\nformat binary_big_endian 1.0\ncomment made by hand\nelement vertex 3\nproperty double x\nproperty double y\n"
            b"property double z\nproperty float nx\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
            b"element face 1\nproperty list uchar int vertex_indices\nend_header\n")
    body = b"".join(struct.pack(">dddfBBB", *[float(v) for v in p], 0.5, *[int(c) for c in col]) for p, col in zip(XYZ, RGB))
    (tmp_path / "be.ply").write_bytes(head + body + struct.pack(">Biii", 3, 0, 1, 2))
    xyz, rgb = pointcloud.load_ply_xyz_rgb(str(tmp_path / "be.ply"))
    assert np.array_equal(xyz, XYZ) and np.array_equal(rgb, RGB)
    # a list element in front of the vertices, little-endian
    head = (b"ply\nformat binary_little_endian 1.0\nelement face 2\nproperty list uchar int vertex_indices\nelement vertex 3\n"
            b"property float x\nproperty float y\nproperty float z\nend_header\n")
    body = struct.pack("<Biii", 3, 0, 1, 2) + struct.pack("<Bii", 2, 0, 1) + XYZ.tobytes()
    (tmp_path / "faces_first.ply").write_bytes(head + body)
    xyz, rgb = pointcloud.load_ply_xyz_rgb(str(tmp_path / "faces_first.ply"))
    assert np.array_equal(xyz, XYZ) and np.array_equal(rgb, np.full((3, 3), 255, np.uint8))       # no colour: white
    # ASCII with r / g / b
    text = "ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\nproperty uchar r\n" \
           "property uchar g\nproperty uchar b\nend_header\n"
    text += "".join(f"{float(p[0])!r} {float(p[1])!r} {float(p[2])!r} {c[0]} {c[1]} {c[2]}\n" for p, c in zip(XYZ, RGB))
    (tmp_path / "ascii.ply").write_text(text)
    xyz, rgb = pointcloud.load_ply_xyz_rgb(str(tmp_path / "ascii.ply"))
    assert np.array_equal(xyz, XYZ) and np.array_equal(rgb, RGB)


def test_reader_colour_rules(tmp_path, gold):
    def write(fields, columns):
        head = "ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
        head += "".join(f"property float {f}\n" for f in fields) + "end_header\n"
        rows = np.concatenate([XYZ, np.asarray(columns, dtype=np.float32)], axis=1).astype("<f4")
        path = tmp_path / ("_".join(fields) + ".ply")
        path.write_bytes(head.encode() + rows.tobytes())
        return pointcloud.load_ply_xyz_rgb(str(path))[1]
    unit = gold["color/unit"][:3]
    assert np.array_equal(write(("red", "green", "blue"), unit), pointcloud._float_rgb_to_u8(unit))
    wide = gold["color/wide"][:3]
    assert np.array_equal(write(("diffuse_red", "diffuse_green", "diffuse_blue"), wide), pointcloud._float_rgb_to_u8(wide))
    dc = gold["color/dc"][:3]
    assert np.array_equal(write(("f_dc_0", "f_dc_1", "f_dc_2"), dc), gold["color/dc_rgb"][:3])
    for bad in (b"plx\n", b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\n"):
        (tmp_path / "bad.ply").write_bytes(bad)
        with pytest.raises(ValueError):
            pointcloud.load_ply_xyz_rgb(str(tmp_path / "bad.ply"))
    (tmp_path / "noxyz.ply").write_bytes(b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nend_header\n1.0\n")
    with pytest.raises(ValueError):
        pointcloud.load_ply_xyz_rgb(str(tmp_path / "noxyz.ply"))


def test_colour_conversions_equal_the_reference(gold):
    assert np.array_equal(pointcloud.convert_3dgs_dc_to_rgb8(gold["color/dc"]), gold["color/dc_rgb"])
    assert np.array_equal(pointcloud._float_rgb_to_u8(gold["color/unit"]), gold["color/unit_rgb"])
    assert np.array_equal(pointcloud._float_rgb_to_u8(gold["color/wide"]), gold["color/wide_rgb"])
    assert np.array_equal(pointcloud._float_rgb_to_u8(np.full((2, 3), np.nan, np.float32)), np.zeros((2, 3), np.uint8))


def test_sky_points_equal_the_reference(gold):
    for i, (row, axis) in enumerate(zip(gold["sky/params"], gold["sky/axes"])):
        centre, scale, count, percent, colour = row[:3].astype(np.float32), float(row[3]), int(row[4]), float(row[5]), row[6:9].astype(np.uint8)
        pts, cols = pointcloud._generate_sky_points(centre, pointcloud._axis_direction(str(axis)), scale, count, colour, sky_percent=percent)
        assert pts.dtype == np.float32 and cols.dtype == np.uint8
        assert np.array_equal(pts, gold[f"sky/{i}/xyz"]) and np.array_equal(cols, gold[f"sky/{i}/rgb"])
    assert pointcloud._axis_direction("up") is None
    assert np.array_equal(pointcloud._parse_sky_color("#fa0"), [255, 170, 0]) and np.array_equal(pointcloud._parse_sky_color("300, 2.9,-1"), [255, 2, 0])
    for text, why in (("1,2", "expected R,G,B components"), ("#12345", "hex color must be #RGB or #RRGGBB"), ("blue", "use #RRGGBB or R,G,B format")):
        with pytest.raises(ValueError, match=why):
            pointcloud._parse_sky_color(text)


def test_searches_skip_without_a_device(gold, capsys):
    """a target outside (0, n) returns the input and never opens the GPU"""
    xyz, rgb = gold["mix/xyz"][:50], gold["mix/rgb"][:50]
    out = pointcloud.voxel_downsample_to_target(xyz, rgb, 50, return_indices=True)
    assert np.array_equal(out[2], np.arange(50)) and out[0] is xyz
    assert capsys.readouterr().out == ("[target] input_points=50  target=50  tol=+/-2.0%  max_iter=32\n"
                                       "[target] skip: target=50 is out of range (output = input)\n")
    out = pointcloud.spatial_hash_downsample_one_pass(xyz, rgb, target_points=80)
    assert len(out) == 2 and capsys.readouterr().out == "[spatial-hash] skip: target=50 is not smaller than input=50\n"
    pointcloud.spatial_hash_downsample_one_pass(xyz, rgb)
    assert capsys.readouterr().out == "[spatial-hash] skip (no voxel-size/target-points)\n"
    empty = pointcloud.voxel_downsample_by_size(xyz[:0], rgb[:0], 0.5, return_indices=True)
    assert empty[2].shape == (0,) and empty[2].dtype == np.int64
