"""VOX-SPEC v1 on the device (csrc/gs360_voxel.hip through gs360/pointcloud.py): bounds, counts and pick indices equal the NumPy
restatement (tests/voxel_np.py) bit for bit; the searches print the reference's recorded lines and return its picks."""
import numpy as np
import pytest

import voxel_np
from conftest import GOLDEN
from gs360 import capi, pointcloud

pytestmark = pytest.mark.gpu
STRATEGIES = ("first", "center", "centroid")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN / "plyopt_goldens.npz")


def check(ctx, xyz, voxels, slot=0, strategies=STRATEGIES):
    """every device result on `xyz` at every voxel size against the restatement"""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    minmax = voxel_np.bounds(xyz)
    with pointcloud.Cloud(ctx, xyz, slot=slot) as cloud:
        assert cloud.minmax.dtype == np.float32 and np.array_equal(cloud.minmax, minmax)
        for voxel in voxels:
            assert voxel_np.layout(minmax, voxel) is not None, "this case is meant for the device path"
            want_k, _packed = voxel_np.unique_count(xyz, voxel, minmax)
            assert cloud.unique_count(voxel) == want_k, voxel
            for how in strategies:
                got = cloud.downsample_by_size(voxel, how)
                assert got.dtype == np.int64 and np.array_equal(got, voxel_np.pick(xyz, voxel, how, minmax)), (voxel, how)
            got = cloud.downsample_by_size(voxel, "random")
            keys = voxel_np.packed_keys(xyz, minmax, voxel)
            assert got.shape == (want_k,) and np.array_equal(keys[got], np.unique(keys)), voxel   # one pick in every voxel, in key order
            assert np.array_equal(cloud.downsample_by_size(voxel, "first", return_indices=False), xyz[voxel_np.pick(xyz, voxel, "first", minmax)])


@pytest.mark.parametrize("name", ["mix", "long"])
def test_golden_clouds(ctx, gold, name):
    check(ctx, gold[f"{name}/xyz"], [float(v) for v in gold[f"{name}/voxels"]])
    for vi, voxel in enumerate(gold[f"{name}/voxels"]):     # and the reference's own picks, for the record of what is compared
        assert np.array_equal(voxel_np.pick(gold[f"{name}/xyz"], float(voxel), "centroid"), gold[f"{name}/pick/{vi}/centroid"])


def test_one_point_and_two_identical_points(ctx):
    check(ctx, [[1.5, -2.0, 3.25]], [0.5, 1e-3])
    check(ctx, [[1.5, -2.0, 3.25], [1.5, -2.0, 3.25]], [0.5])
    check(ctx, [[0.0, 0.0, 0.0], [-0.0, 0.0, 1.0], [0.0, -0.0, 1.0]], [0.25, 1.0, 2.0])


def test_4097_points_in_one_voxel(ctx):
    """a segment longer than a workgroup: the wavefront's float64 sum runs in segment order over 64 full fetches and one of a
    single point; magnitudes 33 bits apart make the order matter"""
    rng = np.random.default_rng(4097)
    xyz = (rng.uniform(-1.0, 1.0, size=(4097, 3)) * 10.0 ** rng.integers(-6, 5, size=(4097, 3))).astype(np.float32)
    assert voxel_np.unique_count(xyz, 1e5)[0] == 1
    check(ctx, xyz, [1e5])


def test_4097_points_in_4097_voxels(ctx):
    rng = np.random.default_rng(7)
    cells = 1 + rng.permutation(17 ** 3 - 1)[:4096]       # 4096 other cells of a 17^3 grid, and the origin in its own
    xyz = np.stack([cells // 289, (cells // 17) % 17, cells % 17], axis=1) + rng.uniform(0.1, 0.9, size=(4096, 3))
    xyz = np.concatenate([xyz[:1000], [[0.0, 0.0, 0.0]], xyz[1000:]])
    assert voxel_np.unique_count(xyz.astype(np.float32), 1.0)[0] == 4097
    check(ctx, xyz, [1.0])


def test_segments_around_the_lane_and_wavefront_paths(ctx):
    """voxels of 1, 2, 31, 32, 33, 63, 64, 65, 128 and 129 points: a lane picks up to 32, its wavefront the longer ones"""
    rng = np.random.default_rng(33)
    sizes = [1, 2, 31, 32, 33, 63, 64, 65, 128, 129, 5, 40]
    xyz = np.concatenate([np.array([3.0 * c, 2.0 * (c % 3), 0.0]) + rng.uniform(0.05, 0.95, size=(s, 3)) for c, s in enumerate(sizes)])
    xyz = xyz[rng.permutation(xyz.shape[0])]
    check(ctx, xyz, [1.0])
    ties = np.repeat(xyz[:7], 50, axis=0)                   # every distance tied: the smallest index wins on either path
    check(ctx, ties[rng.permutation(ties.shape[0])], [1.0, 100.0])


def test_70000_points(ctx):
    """more than one sort block, more than one digit pass, 35 head tiles"""
    rng = np.random.default_rng(70000)
    xyz = rng.normal(size=(70000, 3)) * np.array([30.0, 8.0, 2.0])
    check(ctx, xyz, [0.05, 0.7, 9.0])


def test_voxel_equal_to_the_extent(ctx):
    """the maximum point lies on the upper face: its key is 1 on every axis"""
    rng = np.random.default_rng(5)
    xyz = np.concatenate([rng.uniform(0.0, 1.0, size=(300, 3)), [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [1.0, 0.25, 0.0]]]).astype(np.float32)
    assert voxel_np.layout(voxel_np.bounds(xyz), 1.0) == [1, 1, 1]
    check(ctx, xyz, [1.0, 0.5])


def test_a_grid_too_fine_for_packed_keys(ctx, gold):
    xyz = gold["mix/xyz"]
    minmax = voxel_np.bounds(xyz)
    assert voxel_np.layout(minmax, 1e-7) is None
    with pointcloud.Cloud(ctx, xyz) as cloud:
        pick = ctx.alloc(4 * cloud.n)
        for call in (lambda: ctx.voxel_count_dev(cloud.d_xyz, cloud.n, cloud.minmax, 1e-7, cloud.scratch),
                     lambda: ctx.voxel_pick_dev(cloud.d_xyz, cloud.n, cloud.minmax, 1e-7, capi.VOXEL_FIRST, cloud.scratch, pick)):
            with pytest.raises(capi.Gs360Error) as e:
                call()
            assert e.value.code == capi.ERR_UNSUPPORTED
        ctx.free(pick)
        for voxel in (1e-7, 1e-9):
            assert cloud.unique_count(voxel) == voxel_np.unique_count(xyz, voxel, minmax)[0]
        for how in STRATEGIES:
            assert np.array_equal(cloud.downsample_by_size(1e-7, how), pointcloud._host_pick(xyz, 1e-7, minmax[:3], how))
        got = cloud.downsample_by_size(1e-7, "random")
        keys = voxel_np.triple_keys(xyz, minmax, 1e-7)
        assert np.array_equal(keys[got], np.unique(keys, axis=0))


def test_refusals(ctx, gold):
    xyz = gold["mix/xyz"][:500].copy()
    for bad in (np.nan, np.inf, -np.inf):
        broken = xyz.copy()
        broken[123, 1] = bad
        with pytest.raises(capi.Gs360Error) as e:
            pointcloud.Cloud(ctx, broken)
        assert e.value.code == capi.ERR_ARG and "non-finite" in e.value.text
    with pointcloud.Cloud(ctx, xyz) as cloud:
        inner = cloud.minmax.copy()
        inner[3] = np.float32(0.5) * (inner[0] + inner[3])  # bounds that do not bound the cloud
        with pytest.raises(capi.Gs360Error) as e:
            ctx.voxel_count_dev(cloud.d_xyz, cloud.n, inner, 0.5, cloud.scratch)
        assert e.value.code == capi.ERR_ARG
        small = ctx.alloc(4096)
        with pytest.raises(capi.Gs360Error) as e:
            ctx.voxel_count_dev(cloud.d_xyz, cloud.n, cloud.minmax, 0.5, small)
        assert e.value.code == capi.ERR_ARG
        ctx.free(small)
        for voxel in (0.0, -1.0):
            with pytest.raises(ValueError, match="voxel must be > 0"):
                cloud.unique_count(voxel)
        with pytest.raises(ValueError, match="Unknown representative strategy: nearest"):
            cloud.downsample_by_size(0.5, "nearest")
        assert cloud.unique_count(np.float64(0.5)) == cloud.unique_count(0.5) == voxel_np.unique_count(xyz, 0.5)[0]


def test_a_non_default_slot(ctx, gold):
    check(ctx, gold["long/xyz"], [0.5], slot=1)


@pytest.mark.parametrize("target", [400, 1500, 3899])
def test_target_search_prints_and_picks_what_the_reference_does(ctx, gold, capsys, target):
    xyz, rgb = gold["mix/xyz"], gold["mix/rgb"]
    with pointcloud.Cloud(ctx, xyz) as cloud:
        out = pointcloud.voxel_downsample_to_target(xyz, rgb, target, return_indices=True, cloud=cloud)
        assert capsys.readouterr().out == str(gold[f"mix/target/{target}/stdout"])
        want = gold[f"mix/target/{target}/pick"]
        assert np.array_equal(out[2], want) and np.array_equal(out[0], xyz[want]) and np.array_equal(out[1], rgb[want])
        assert out[0].dtype == np.float32 and out[1].dtype == np.uint8 and out[2].dtype == np.int64
        out = pointcloud.spatial_hash_downsample_one_pass(xyz, rgb, target_points=target, return_indices=True, cloud=cloud)
        assert capsys.readouterr().out == str(gold[f"mix/hash/{target}/stdout"])
        assert np.array_equal(out[2], gold[f"mix/hash/{target}/pick"])
        assert len(pointcloud.spatial_hash_downsample_one_pass(xyz, rgb, voxel_size=0.5, cloud=cloud)) == 2
        assert capsys.readouterr().out == f"[spatial-hash] fixed voxel-size=0.5\n[spatial-hash] voxel=0.5  out_points={int(gold['mix/counts'][2]):,} (approx)\n"


def test_module_functions_make_their_own_cloud(gold):
    """without `cloud=`: the module's default context, opened on first use and closed on request"""
    xyz, rgb = gold["long/xyz"], gold["long/rgb"]
    try:
        out = pointcloud.voxel_downsample_by_size(xyz, rgb, 0.5, representative="center", return_indices=True)
        assert np.array_equal(out[2], gold["long/pick/1/center"])
        out = pointcloud.voxel_downsample_by_size(xyz, rgb, 0.25)
        assert len(out) == 2 and np.array_equal(out[0], xyz[gold["long/pick/0/centroid"]])
    finally:
        pointcloud.close_default_context()
