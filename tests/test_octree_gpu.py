"""OCT-SPEC v1 on the device (csrc/gs360_octree.hip through gs360/pointcloud.py): the kept leaves' pick indices equal the unmodified
reference's on its golden grid (tests/golden/octree_goldens.npz) and the NumPy restatement's (tests/octree_np.py) on clouds at the
spec's edges, index for index and in output order."""
import numpy as np
import pytest

import octree_cases
import octree_np
from conftest import GOLDEN
from gs360 import capi, pointcloud

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN / "octree_goldens.npz")


def test_golden_grid(ctx, gold):
    """all 270 cases of the reference: targets 1 .. n - 1, five weights, with and without a smallest voxel, three strategies"""
    xyz = gold["mix/xyz"]
    with pointcloud.Cloud(ctx, xyz) as cloud:
        for ti, target in enumerate(gold["mix/targets"]):
            for wi, weight in enumerate(gold["mix/weights"]):
                for vi, min_voxel in enumerate(gold["mix/min_voxels"]):
                    for how in octree_cases.STRATEGIES:
                        got = cloud.adaptive_downsample(int(target), float(weight), float(min_voxel) or None, how)
                        assert got.dtype == np.int64 and np.array_equal(got, gold[f"mix/pick/{ti}/{wi}/{vi}/{how}"]), (target, weight, min_voxel, how)


def test_one_wavefront_walks_leaves_of_tens_of_thousands(ctx, gold):
    xyz = gold["big/xyz"]
    with pointcloud.Cloud(ctx, xyz) as cloud:
        for ti, target in enumerate(gold["big/targets"]):
            for how in octree_cases.STRATEGIES:
                assert np.array_equal(cloud.adaptive_downsample(int(target), representative=how), gold[f"big/pick/{ti}/{how}"]), (target, how)


@pytest.mark.parametrize("case", octree_cases.cases(), ids=lambda c: c[0])
def test_edge_clouds(ctx, case):
    name, xyz, runs = case
    with pointcloud.Cloud(ctx, xyz) as cloud:
        for target, power, min_voxel in runs:
            for how in octree_cases.STRATEGIES:
                got = cloud.adaptive_downsample(target, power, min_voxel, how)
                assert np.array_equal(got, octree_np.pick(xyz, target, power, min_voxel, how)), (name, target, power, min_voxel, how)


def test_262147_points_at_ten_percent(ctx):
    """several tiles of both sorts and of the per-point passes, and a tail of three points behind the last whole lane"""
    rng = np.random.default_rng(262147)
    n = 262147
    d = rng.normal(size=(n, 3))
    xyz = (d / np.linalg.norm(d, axis=1, keepdims=True) * [6.0, 4.0, 1.5] + rng.normal(size=(n, 3)) * 0.02).astype(np.float32)
    with pointcloud.Cloud(ctx, xyz) as cloud:
        for how in octree_cases.STRATEGIES:
            got = cloud.adaptive_downsample(n // 10 + 1, representative=how)
            assert got.shape == (n // 10 + 1,) and np.array_equal(got, octree_np.pick(xyz, n // 10 + 1, how=how)), how


def test_random_returns_one_member_of_every_kept_leaf(ctx, gold):
    xyz = gold["mix/xyz"]
    with pointcloud.Cloud(ctx, xyz) as cloud:
        for target, power, min_voxel in ((9, 1.0, None), (230, 0.5, 0.75), (1000, 2.0, None), (2299, 1.0, None)):
            got = cloud.adaptive_downsample(target, power, min_voxel, "random")
            segs = octree_np.segments(xyz, target, power, min_voxel)[0]
            assert got.dtype == np.int64 and got.shape == (len(segs),)
            assert all(pick in idx for pick, (idx, _d) in zip(got.tolist(), segs)), (target, power, min_voxel)


def test_module_function_and_a_second_slot(ctx, gold):
    xyz, rgb = gold["mix/xyz"], gold["mix/rgb"]
    want = gold["mix/pick/5/0/0/centroid"]                   # target 50, weight 1, no smallest voxel
    with pointcloud.Cloud(ctx, xyz, slot=1) as cloud:
        assert np.array_equal(cloud.adaptive_downsample(50), want)
        out = pointcloud.adaptive_voxel_downsample(xyz, rgb, 50, return_indices=True, cloud=cloud)
        assert np.array_equal(out[2], want) and np.array_equal(out[0], xyz[want]) and np.array_equal(out[1], rgb[want])
        stats = pointcloud.compute_point_cloud_stats(xyz)
        out = pointcloud.adaptive_voxel_downsample(xyz, rgb, 50, 1.0, stats, None, "centroid", 12, cloud=cloud)
        assert len(out) == 2 and np.array_equal(out[0], xyz[want])
        assert np.array_equal(cloud.downsample_by_size(0.5, "first"), pointcloud._host_pick(xyz, 0.5, cloud.minmax[:3], "first"))   # the voxel calls still run
    try:
        out = pointcloud.adaptive_voxel_downsample(xyz, rgb, 50, return_indices=True)      # a cloud of its own on the default context
    finally:
        pointcloud.close_default_context()
    assert np.array_equal(out[2], want)


def test_refusals(ctx, gold):
    xyz = gold["mix/xyz"][:500].copy()
    cube_min, cube_size = octree_np.cube(xyz)
    with pointcloud.Cloud(ctx, xyz) as cloud:
        with pytest.raises(ValueError, match="Unknown representative strategy: nearest"):
            cloud.adaptive_downsample(10, representative="nearest")
        with pytest.raises(capi.Gs360Error) as e:
            pointcloud.adaptive_voxel_downsample(xyz, np.zeros((500, 3), np.uint8), 10, max_depth=10, cloud=cloud)
        assert e.value.code == capi.ERR_UNSUPPORTED
        with pytest.raises(capi.Gs360Error) as e:
            cloud.adaptive_downsample(10, weight_power=1e6)       # 500 ** 1e6: Python raises OverflowError there
        assert e.value.code == capi.ERR_UNSUPPORTED
        scratch = ctx.alloc(ctx.octree_scratch(500))
        call = lambda **kw: ctx.octree_pick_dev(**{**dict(xyz=cloud.d_xyz, n=500, cube_min=cube_min, cube_size=cube_size, target=10, weight_power=1.0,
                                                          min_voxel=0.0, strategy=capi.VOXEL_FIRST, scratch=scratch), **kw})
        assert np.array_equal(call()[0], octree_np.pick(xyz, 10, how="first"))
        small = ctx.alloc(4096)
        for kw in (dict(target=0), dict(target=500), dict(n=1, target=1), dict(cube_size=0.0), dict(cube_size=np.inf), dict(weight_power=np.nan),
                   dict(cube_min=[0.0, np.nan, 0.0]), dict(strategy=4), dict(strategy=capi.VOXEL_SEGMENTS), dict(scratch=small), dict(slot=7)):
            with pytest.raises(capi.Gs360Error) as e:
                call(**kw)
            assert e.value.code == capi.ERR_ARG, kw
        ctx.free(small)
        ctx.free(scratch)
        with pytest.raises(capi.Gs360Error) as e:
            ctx.octree_scratch(1)
        assert e.value.code == capi.ERR_ARG
        with pytest.raises(capi.Gs360Error) as e:
            ctx.octree_scratch(1 << 31)
        assert e.value.code == capi.ERR_UNSUPPORTED
