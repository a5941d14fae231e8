"""gs360_PlyOptimizer.py without a GPU: the reference's parser errors (PLY:1571-1586), the statistics-only run (PLY:1604-1654), the
refusals of what is not built, and a downsampling run on a machine without a device."""
import numpy as np
import pytest

import gs360_PlyOptimizer as tool
from gs360 import pointcloud

XYZ = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 4.0], [0.5, 1.0, 1.0], [1.0, 0.0, 0.0]], dtype=np.float32)
RGB = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12]], dtype=np.uint8)
AABB = "[aabb] min=(0, 0, 0)  max=(1, 2, 4)  extent=(1, 2, 4)  volume~8"


@pytest.fixture
def ply(tmp_path):
    path = tmp_path / "cloud.ply"
    pointcloud.save_ply_binary_little(str(path), XYZ, RGB)
    return path


@pytest.mark.parametrize("extra,message", [
    (["-t", "0"], "--target-points must be greater than 0"),
    (["-t", "-5"], "--target-points must be greater than 0"),
    (["--sky-axis", "+Z", "--sky-scale", "0"], "--sky-scale must be > 0 when --sky-axis is set"),
    (["--sky-axis", "+Z", "--sky-count", "0"], "--sky-count must be > 0 when --sky-axis is set"),
    (["--sky-axis=-X", "--sky-percent", "0"], "--sky-percent must be > 0 and <= 100 when --sky-axis is set"),
    (["--sky-axis=-X", "--sky-percent", "100.5"], "--sky-percent must be > 0 and <= 100 when --sky-axis is set"),
    (["--sky-axis", "+Y", "--sky-color", "1,2"], "--sky-color expected R,G,B components"),
    (["--sky-axis", "+Y", "--sky-color", "#1234"], "--sky-color hex color must be #RGB or #RRGGBB"),
    (["--sky-axis", "+Y", "--sky-color", "sky"], "--sky-color use #RRGGBB or R,G,B format"),
    (["--sky-axis", "up"], "invalid choice"),
    (["-k", "nearest"], "invalid choice"),
    (["--downsample-method", "octree"], "invalid choice"),
])
def test_parser_errors(ply, capsys, extra, message):
    with pytest.raises(SystemExit) as e:
        tool.main(["-i", str(ply)] + extra)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert message in err and err.startswith("usage: PointCloudOptimizer")


def test_input_is_required(capsys):
    with pytest.raises(SystemExit) as e:
        tool.main(["-o", "out.ply"])
    assert e.value.code == 2 and "-i/--in" in capsys.readouterr().err


def test_defaults_are_the_reference_s():
    args = tool.create_arg_parser().parse_args(["-i", "x.ply"])
    assert (args.output, args.target_points, args.target_percent, args.voxel_size) == (None, None, None, None)
    assert (args.downsample_method, args.adaptive, args.adaptive_weight, args.append_ply, args.keep_strategy) == ("voxel", False, 1.0, [], "centroid")
    assert (args.sky_axis, args.sky_scale, args.sky_count, args.sky_percent, args.sky_color) == (None, 100.0, 4000, 50.0, "#87cefa")
    args = tool.create_arg_parser().parse_args(["--in", "x.ply", "--out", "y.ply", "--target-points", "7", "--target-percent", "2.5", "--voxel-size",
                                                "0.1", "--append-ply", "a.ply", "-a", "b.ply", "--keep-strategy", "random"])
    assert (args.input, args.output, args.target_points, args.target_percent, args.voxel_size) == ("x.ply", "y.ply", 7, 2.5, 0.1)
    assert args.append_ply == ["a.ply", "b.ply"] and args.keep_strategy == "random"


def test_statistics_only(ply, capsys):
    assert tool.main(["-i", str(ply)]) == 0
    assert capsys.readouterr().out.splitlines() == [
        f"[load] kind=ply base={ply.resolve()}  points=4", "input_points=4", AABB, "[init] v0~1.25992  lo=0.0196863  hi=80.6349",
        "[info] --out not provided; statistics only."]


@pytest.mark.parametrize("extra", [["-v", "0.5"], ["-a", "more.ply"], ["--downsample-method", "spatial-hash"], ["--adaptive"],
                                   ["--downsample-method", "adaptive"]])
def test_statistics_only_with_options_that_need_an_output(ply, capsys, extra):
    assert tool.main(["-i", str(ply)] + extra) == 0
    assert capsys.readouterr().out.splitlines() == [
        f"[load] kind=ply base={ply.resolve()}  points=4", "input_points=4", AABB, "[init] v0~1.25992  lo=0.0196863  hi=80.6349",
        "[warn] --out missing; skipping downsample/append options."]


def test_statistics_only_with_a_target(ply, capsys):
    assert tool.main(["-i", str(ply), "-t", "9", "-r", "50"]) == 0
    assert capsys.readouterr().out.splitlines() == [
        f"[load] kind=ply base={ply.resolve()}  points=4", "[target-percent] 50% of 4 -> target_points=2",
        "[target-percent] override replacing explicit target_points=9", "input_points=4", AABB,
        "[warn] --out missing; skipping downsample/append options."]
    assert tool.main(["-i", str(ply), "-r", "0"]) == 0
    assert capsys.readouterr().out.splitlines()[1] == "[target-percent] 0% of 4 -> target_points=0"


@pytest.mark.parametrize("extra", [["--adaptive"], ["--downsample-method", "adaptive", "-t", "2"]])
def test_adaptive_is_refused_before_anything_is_written(ply, tmp_path, capsys, extra):
    out = tmp_path / "out.ply"
    assert tool.main(["-i", str(ply), "-o", str(out)] + extra) == 1
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 1 and lines[0].startswith("[ERR] ") and "adaptive" in lines[0]
    assert not out.exists()


def test_colmap_folder_is_refused(tmp_path, capsys):
    model = tmp_path / "sparse"
    model.mkdir()
    for name in ("cameras.txt", "images.txt", "points3D.txt"):
        (model / name).write_text("# empty\n")
    out = tmp_path / "out"
    assert tool.main(["-i", str(model), "-o", str(out)]) == 1
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 1 and lines[0].startswith("[ERR] ") and "COLMAP" in lines[0]
    assert not out.exists()


def test_no_downsampling_writes_the_cloud_with_appends_and_sky_without_a_device(ply, tmp_path, capsys):
    """no -v / -t: nothing for the GPU to do; append and sky are host work (PLY:1755-1831)"""
    extra = tmp_path / "extra.ply"
    pointcloud.save_ply_binary_little(str(extra), XYZ[:2] + 10, RGB[:2])
    out = tmp_path / "out.ply"
    assert tool.main(["-i", str(ply), "-o", str(out), "-a", "extra.ply", "--sky-axis", "+Z", "--sky-count", "5", "--sky-scale", "2",
                      "--sky-color", "9,8,7"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines[4:] == ["[downsample] skip (no voxel-size/target-points)", f"[append] {extra} +2 -> total 6", "[append] total added: 2",
                         "[sky] axis=+Z scale=2 percent=50 count=5 -> total 11", f"[save] {out}  points=11  (binary little-endian PLY)"]
    xyz, rgb = pointcloud.load_ply_xyz_rgb(str(out))
    both = np.concatenate([XYZ, XYZ[:2] + 10])
    assert np.array_equal(xyz[:6], both) and np.array_equal(rgb[:6], np.concatenate([RGB, RGB[:2]]))
    centre = ((both.min(axis=0) + both.max(axis=0)) * np.float32(0.5)).astype(np.float32)
    sky, cols = pointcloud._generate_sky_points(centre, pointcloud._axis_direction("+Z"), 2.0, 5, np.array([9, 8, 7], np.uint8))
    assert np.array_equal(xyz[6:], sky) and np.array_equal(rgb[6:], cols)


@pytest.mark.parametrize("extra", [["-v", "0.5"], ["-t", "2"], ["-t", "2", "--downsample-method", "spatial-hash"]])
def test_downsampling_without_a_gpu_is_one_error_line(ply, tmp_path, capsys, extra):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here")
    out = tmp_path / "out.ply"
    assert tool.main(["-i", str(ply), "-o", str(out)] + extra) == 1
    errs = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("[ERR]")]
    assert len(errs) == 1 and "gs360 error -3" in errs[0]
    assert not out.exists()
