"""The four-points-per-lane pass of the point-cloud kernels (csrc/gs360_cloudsteps.h: vx_keys_kernel, oc_codes_kernel) on clouds of
5, 6 and 7 points: one whole lane of four points and, directly behind it, a lane with a tail of one, two and three.  Counts and
picks equal the NumPy restatements (tests/voxel_np.py, tests/octree_np.py) index for index."""
import numpy as np
import pytest

import octree_np
import voxel_np
from gs360 import pointcloud

pytestmark = pytest.mark.gpu
STRATEGIES = ("first", "center", "centroid")
VOXELS = (0.5, 4.0)                                        # nearly every point in a voxel of its own; several points in a voxel


@pytest.fixture(scope="module")
def points():
    return (np.random.default_rng(567).normal(size=(7, 3)) * np.array([3.0, 2.0, 1.0])).astype(np.float32)


@pytest.mark.parametrize("n", [5, 6, 7])
def test_tail_behind_one_whole_lane(ctx, points, n):
    xyz = np.ascontiguousarray(points[:n])
    minmax = voxel_np.bounds(xyz)
    assert voxel_np.unique_count(xyz, VOXELS[1], minmax)[0] < voxel_np.unique_count(xyz, VOXELS[0], minmax)[0] <= n
    with pointcloud.Cloud(ctx, xyz) as cloud:
        for voxel in VOXELS:
            assert cloud.unique_count(voxel) == voxel_np.unique_count(xyz, voxel, minmax)[0], voxel
            for how in STRATEGIES:
                assert np.array_equal(cloud.downsample_by_size(voxel, how), voxel_np.pick(xyz, voxel, how, minmax)), (voxel, how)
        for target in (2, n - 1):
            for how in STRATEGIES:
                got = cloud.adaptive_downsample(target, representative=how)
                assert np.array_equal(got, octree_np.pick(xyz, target, how=how)), (target, how)
