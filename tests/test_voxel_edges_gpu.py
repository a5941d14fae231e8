"""VOX-SPEC v1 on the device where real clouds take it and tests/test_voxel_gpu.py does not: more than 2^21 points (a scan chunk above
one tile per lane, the capped bounds grid), packed keys of up to 64 bits, points on computed faces of voxels that are no power of
two, squared distances that are subnormal or infinite on either pick path, and the segment arrays themselves.  Everything equals the
NumPy restatement (tests/voxel_np.py) bit for bit; what a case promises about its path is asserted from the restatement
(tests/voxel_cases.py builds the clouds)."""
import numpy as np
import pytest

import voxel_cases
import voxel_np
from conftest import GOLDEN
from gs360 import capi, pointcloud
from test_voxel_gpu import check

pytestmark = pytest.mark.gpu
STRATEGIES = ("first", "center", "centroid")
PAD, FILL = 64, 0xA5                                       # entries behind every output, and the byte they must keep


class Outputs:
    """pick, order and starts buffers of n + PAD entries, filled with a pattern in front of every call"""

    def __init__(self, ctx, n, slot=0):
        self.ctx, self.n, self.slot = ctx, n, slot
        self.bufs = [ctx.alloc(4 * (n + PAD)) for _ in range(3)]

    def close(self):
        for b in self.bufs:
            self.ctx.free(b)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def call(self, cloud, voxel, strategy, use):
        """one gs360_voxel_pick_f32 with the outputs named in `use` -> (k, {name: the whole buffer})"""
        for b in self.bufs:
            self.ctx.memset(b, FILL, self.slot)
        given = [b if name in use else None for name, b in zip(("pick", "order", "starts"), self.bufs)]
        k = self.ctx.voxel_pick_dev(cloud.d_xyz, cloud.n, cloud.minmax, voxel, strategy, cloud.scratch, *given, self.slot)
        return k, {name: self.ctx.download(b, (self.n + PAD,), np.uint32, self.slot) for name, b in zip(("pick", "order", "starts"), self.bufs)}


def untouched(a):
    return bool(np.all(a.view(np.uint8) == FILL))


def check_segments(ctx, cloud, voxel, want=None, strategy=capi.VOXEL_SEGMENTS, want_pick=None):
    """the order and starts arrays of one call (and its picks, under a pick strategy) against the restatement's, and every byte
    behind them against the pattern; want = voxel_np.segments(...)"""
    _ks, order, starts, _bits = voxel_np.segments(cloud.xyz, voxel) if want is None else want
    n, k = cloud.n, starts.size
    with Outputs(ctx, n, cloud.slot) as out:
        got_k, got = out.call(cloud, voxel, strategy, ("order", "starts") if strategy == capi.VOXEL_SEGMENTS else ("pick", "order", "starts"))
    assert got_k == k
    assert np.array_equal(got["order"][:n], order) and untouched(got["order"][n:])
    assert np.array_equal(got["starts"][:k], starts) and untouched(got["starts"][k:])
    if strategy == capi.VOXEL_SEGMENTS:
        assert untouched(got["pick"])
    else:
        assert np.array_equal(got["pick"][:k], want_pick) and untouched(got["pick"][k:])


# ---- 1. clouds above 2 097 152 points ------------------------------------------------------------------------------------------------
BIG_VOXELS = (0.35, 0.02)


@pytest.fixture(scope="module")
def big(ctx):
    xyz = voxel_cases.clustered_cloud()
    with pointcloud.Cloud(ctx, xyz) as cloud:
        yield cloud


@pytest.fixture(scope="module")
def big_segments(big):
    """voxel -> voxel_np.segments of the clustered cloud, made once"""
    made = {}

    def get(voxel):
        if voxel not in made:
            made[voxel] = voxel_np.segments(big.xyz, voxel)
        return made[voxel]
    return get


def test_clustered_cloud_bounds(ctx, big):
    n = big.n
    assert n == voxel_cases.BIG_N and n % 4 != 0
    assert n > 1024 * voxel_cases.BOUND_BLOCKS and -(-n // (4 * voxel_cases.BOUND_THREADS)) > voxel_cases.BOUND_BLOCKS   # the grid is capped
    assert big.minmax.dtype == np.float32 and np.array_equal(big.minmax, voxel_np.bounds(big.xyz))


@pytest.mark.parametrize("voxel", BIG_VOXELS)
def test_clustered_cloud_takes_the_chunked_scan(big, big_segments, voxel):
    """the preconditions of the tests below, from the restatement"""
    ks, _order, starts, _bits = big_segments(voxel)
    tiles = voxel_cases.heads_per_tile(ks)
    assert tiles.size == voxel_cases.n_tiles(big.n) > voxel_cases.SCAN_THREADS
    chunk = -(-tiles.size // voxel_cases.SCAN_THREADS)
    assert chunk == 2 and -(-tiles.size // chunk) < voxel_cases.SCAN_THREADS    # lanes with two tiles, and lanes with none
    assert tiles.min() != tiles.max() and tiles.max() - tiles.min() > 1000
    assert np.diff(np.r_[starts, big.n]).max() > voxel_cases.LANE_MAX


@pytest.mark.parametrize("voxel", BIG_VOXELS)
def test_clustered_cloud_count_and_first(big, big_segments, voxel):
    _ks, order, starts, _bits = big_segments(voxel)
    want_k, packed = voxel_np.unique_count(big.xyz, voxel)
    assert packed and want_k == starts.size
    assert big.unique_count(voxel) == want_k
    got = big.downsample_by_size(voxel, "first")
    assert got.dtype == np.int64 and np.array_equal(got, order[starts]) and np.array_equal(got, voxel_np.pick(big.xyz, voxel, "first"))


@pytest.mark.parametrize("voxel", BIG_VOXELS)
def test_clustered_cloud_centroid(big, voxel):
    assert np.array_equal(big.downsample_by_size(voxel, "centroid"), voxel_np.pick(big.xyz, voxel, "centroid"))


@pytest.mark.parametrize("voxel", BIG_VOXELS)
def test_clustered_cloud_segment_arrays(ctx, big, big_segments, voxel):
    check_segments(ctx, big, voxel, big_segments(voxel))


def test_two_voxels_of_4194305_points(ctx):
    """two heads in 2049 tiles: all but two tiles add zero to the scan, and the first voxel's run crosses every seam between the
    lanes' chunks of three tiles in front of its odd end"""
    head_at = 1025 * voxel_cases.TILE + 777
    xyz = voxel_cases.two_voxel_cloud(head_at)
    minmax = voxel_np.bounds(xyz)
    ks, order, starts, bits = voxel_np.segments(xyz, 1.0, minmax)
    tiles = voxel_cases.heads_per_tile(ks)
    assert bits == [1, 0, 0] and starts.tolist() == [0, head_at] and head_at % 2 == 1
    assert tiles.size == 2049 and -(-tiles.size // voxel_cases.SCAN_THREADS) == 3 and np.count_nonzero(tiles) == 2
    assert (head_at // voxel_cases.TILE) % 3 != 0          # the head is not the first tile of its lane's chunk
    with pointcloud.Cloud(ctx, xyz) as cloud:
        assert np.array_equal(cloud.minmax, minmax)
        assert cloud.unique_count(1.0) == 2
        assert np.array_equal(cloud.downsample_by_size(1.0, "first"), order[starts])


# ---- 2. key layouts up to 64 bits ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", voxel_cases.PACKED_LAYOUTS, ids=lambda b: "+".join(map(str, b)))
def test_packed_layouts_up_to_64_bits(ctx, bits):
    xyz = voxel_cases.lattice(bits)
    assert voxel_np.layout(voxel_np.bounds(xyz), 1.0) == list(bits)
    count, packed = voxel_np.unique_count(xyz, 1.0)
    assert packed and count == np.unique(xyz, axis=0).shape[0] < xyz.shape[0]
    check(ctx, xyz, [1.0])


@pytest.mark.parametrize("bits", voxel_cases.REFUSED_LAYOUTS, ids=lambda b: "+".join(map(str, b)))
def test_layouts_of_65_bits_take_the_host_path(ctx, bits):
    xyz = voxel_cases.lattice(bits)
    minmax = voxel_np.bounds(xyz)
    assert voxel_np.layout(minmax, 1.0) is None
    with pointcloud.Cloud(ctx, xyz) as cloud:
        assert np.array_equal(cloud.minmax, minmax)
        pick = ctx.alloc(4 * cloud.n)
        for call in (lambda: ctx.voxel_count_dev(cloud.d_xyz, cloud.n, cloud.minmax, 1.0, cloud.scratch),
                     lambda: ctx.voxel_pick_dev(cloud.d_xyz, cloud.n, cloud.minmax, 1.0, capi.VOXEL_CENTROID, cloud.scratch, pick)):
            with pytest.raises(capi.Gs360Error) as e:
                call()
            assert e.value.code == capi.ERR_UNSUPPORTED
        ctx.free(pick)
        want_k, packed = voxel_np.unique_count(xyz, 1.0, minmax)
        assert not packed and cloud.unique_count(1.0) == want_k == np.unique(xyz, axis=0).shape[0]
        for how in STRATEGIES:
            assert np.array_equal(cloud.downsample_by_size(1.0, how), pointcloud._host_pick(xyz, 1.0, minmax[:3], how)), how
        keys = voxel_np.triple_keys(xyz, minmax, 1.0)
        assert np.array_equal(keys[cloud.downsample_by_size(1.0, "random")], np.unique(keys, axis=0))


# ---- 3. points on computed faces -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("voxel", voxel_cases.FACE_VOXELS, ids=lambda v: f"{v:.3g}")
def test_points_on_computed_faces(ctx, voxel):
    """the key is one correctly rounded float32 divide: more than 1000 of the x quotients are within one ulp of an integer"""
    xyz = voxel_cases.face_cloud(voxel)
    assert xyz.shape == (2100, 3) and np.array_equal(voxel_np.bounds(xyz)[:3], np.zeros(3, np.float32))
    assert voxel_cases.floors_one_ulp_from_a_face(xyz[:, 0], voxel) >= 1000
    check(ctx, xyz, [voxel], strategies=("first", "center"))


# ---- 4. dist2 at float32's edges -----------------------------------------------------------------------------------------------------
def segment_of(xyz, voxel, how, members):
    """the restatement's squared distances of the voxel that holds the points `members`, in segment order, and its pick"""
    order, starts, gid, dist2 = voxel_np.distances(xyz, voxel, how)
    at = np.flatnonzero(gid == gid[np.flatnonzero(order == members[0])[0]])
    assert np.array_equal(order[at], members)
    return dist2[at], int(voxel_np.pick(xyz, voxel, how)[gid[at[0]]])


@pytest.mark.parametrize("count", [23, 150])
def test_subnormal_squared_distances(ctx, count):
    """a kernel that flushed subnormal numbers would see every distance as 0 and take the voxel's first point"""
    assert (count <= voxel_cases.LANE_MAX) != (count > 64)  # the lane's pick, or its wavefront's over more than one fetch
    xyz, members = voxel_cases.subnormal_cloud(count, seed=count)
    dist2, pick = segment_of(xyz, 1.0, "centroid", members)
    tiny = np.finfo(np.float32).tiny
    assert np.all(dist2 < tiny) and np.count_nonzero(dist2) >= count - 1 and dist2.min() < dist2[0]
    assert pick not in (members[0], members[-1])
    check(ctx, xyz, [1.0])


@pytest.mark.parametrize("count", [20, 100])
def test_infinite_squared_distances(ctx, count):
    """all distances +inf: the smallest index wins; +inf in front of finite ones: the nearest point wins"""
    assert (count <= voxel_cases.LANE_MAX) != (count > 64)
    voxel = 1e20
    xyz, corner, mixed = voxel_cases.overflow_cloud(count, seed=count)
    assert np.all(np.isfinite(xyz))
    for how in ("center", "centroid"):
        dist2, pick = segment_of(xyz, voxel, how, corner)
        assert np.all(np.isposinf(dist2)) and pick == corner[0]
        dist2, pick = segment_of(xyz, voxel, how, mixed)
        assert np.all(np.isposinf(dist2[:count])) and np.all(np.isfinite(dist2[count:])) and pick in mixed[count:]
    check(ctx, xyz, [voxel])


# ---- 5. the segment arrays -----------------------------------------------------------------------------------------------------------
def test_segment_arrays_of_the_golden_cloud_and_a_lattice(ctx):
    gold = np.load(GOLDEN / "plyopt_goldens.npz")
    for xyz, voxels in ((gold["mix/xyz"], [float(v) for v in gold["mix/voxels"]]), (voxel_cases.lattice((32, 0, 32)), [1.0])):
        with pointcloud.Cloud(ctx, xyz) as cloud:
            for voxel in voxels:
                check_segments(ctx, cloud, voxel)


def test_a_pick_strategy_with_all_three_outputs(ctx):
    gold = np.load(GOLDEN / "plyopt_goldens.npz")
    xyz, voxel = gold["mix/xyz"], float(gold["mix/voxels"][1])
    with pointcloud.Cloud(ctx, xyz) as cloud:
        check_segments(ctx, cloud, voxel, strategy=capi.VOXEL_CENTROID, want_pick=voxel_np.pick(xyz, voxel, "centroid"))
