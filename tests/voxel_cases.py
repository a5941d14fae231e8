"""The clouds of tests/test_voxel_edges_gpu.py and of the host check's layout cases (tests/test_voxel_hostcheck.py): a clustered
cloud past every single-chunk path of the head scan and the bounds grid, lattices whose keys fill a chosen number of bits per axis,
points on computed voxel faces, and voxels whose squared distances are subnormal or infinite.  NumPy only; what a case promises
(its path, its bit lengths, its ties) is asserted where it is used, from the restatement (tests/voxel_np.py)."""
import numpy as np

TILE, SCAN_THREADS, BOUND_BLOCKS, BOUND_THREADS, LANE_MAX = 2048, 1024, 1024, 256, 32   # kVxTile, kVxScanThreads, kVxBoundBlocks,
#                                                             kVxThreads of csrc/gs360_voxel.h, kCloudLaneMax of csrc/gs360_cloudsteps.h
BIG_N = 2 * 1024 * 1024 + 2048 + 3         # 1026 tiles: a scan chunk of 2 with idle lanes, a capped bounds grid, a key tail of 3
TWO_VOXEL_N = 2 * 1024 * 2048 + 1          # 2049 tiles: a scan chunk of 3
PACKED_LAYOUTS = ((22, 21, 21), (0, 24, 24), (0, 32, 32), (32, 0, 32), (63, 1, 0), (1, 0, 63), (0, 1, 63))
REFUSED_LAYOUTS = ((23, 21, 21), (21, 22, 22))   # 65 bits: the host path
FACE_VOXELS = (0.1, 0.7, 1.0 / 3.0, 0.013, 5.3)


def n_tiles(n):
    return (n + TILE - 1) // TILE


def heads_per_tile(sorted_keys):
    """what phase 0 of the head pass counts: the keys of every tile of TILE that differ from their predecessor"""
    head = np.r_[True, sorted_keys[1:] != sorted_keys[:-1]]
    return np.add.reduceat(head.astype(np.int64), np.arange(0, sorted_keys.size, TILE))


def clustered_cloud():
    """BIG_N points around 600 centres at three very different spreads: the heads per tile of its sorted keys vary widely"""
    rng = np.random.default_rng(BIG_N)
    centres = rng.uniform(-40.0, 40.0, size=(600, 3))
    xyz = centres[rng.integers(0, 600, BIG_N)] + rng.normal(size=(BIG_N, 3)) * rng.choice([0.02, 0.5, 6.0], size=(BIG_N, 1))
    return xyz.astype(np.float32)


def two_voxel_cloud(head_at):
    """TWO_VOXEL_N shuffled points in two voxels of edge 1.0; the second voxel's head lies at sorted position `head_at`"""
    rng = np.random.default_rng(TWO_VOXEL_N)
    xyz = rng.uniform(0.0, 0.5, size=(TWO_VOXEL_N, 3)).astype(np.float32)
    member = rng.permutation(TWO_VOXEL_N)
    xyz[member[head_at:], 0] += np.float32(1.0)
    xyz[member[0]] = 0.0                                    # the minimum of the cloud
    return xyz


def lattice(bits, seed=None, m=300):
    """integer coordinates (voxel 1.0) whose largest keys have exactly `bits` bits per axis: m random lattice points, 40 exact
    duplicates of them, the top corner and the origin.  An axis of b > 24 bits steps by 2^(b - 24), so that every coordinate is
    exact in float32; an axis of 0 bits is constant."""
    rng = np.random.default_rng(sum(bits) if seed is None else seed)
    steps = [1 << max(b - 24, 0) for b in bits]
    tops = [(1 << b) - s if b else 0 for b, s in zip(bits, steps)]
    pts = np.stack([rng.integers(0, t // s + 1, m) * s for t, s in zip(tops, steps)], axis=1).astype(np.float64)
    pts = np.concatenate([pts, pts[:40], [np.array(tops, dtype=np.float64)], [[0.0, 0.0, 0.0]]])
    xyz = pts.astype(np.float32)
    assert np.array_equal(xyz.astype(np.float64), pts)
    return xyz


def face_cloud(voxel):
    """x on the computed faces float32(k) * float32(voxel), k < 700, and one ulp to either side of them; y and z spread over a few
    voxels; the origin, so that the grid starts at 0"""
    v = np.float32(voxel)
    face = np.arange(700, dtype=np.float32) * v
    x = np.concatenate([np.nextafter(face, np.float32(-np.inf)), face, np.nextafter(face, np.float32(np.inf))])
    x = x[x >= 0]
    rng = np.random.default_rng(700)
    yz = (rng.uniform(0.0, 2.5, size=(x.size, 2)) * float(v)).astype(np.float32)
    xyz = np.concatenate([np.column_stack([x, yz]), np.zeros((1, 3), dtype=np.float32)]).astype(np.float32)
    return xyz[rng.permutation(xyz.shape[0])]


def floors_one_ulp_from_a_face(x, voxel):
    """how many of the float32 quotients x / voxel change their floor when moved by one ulp"""
    q = np.asarray(x, dtype=np.float32) / np.float32(voxel)
    up, down = np.nextafter(q, np.float32(np.inf)), np.nextafter(q, np.float32(-np.inf))
    return int(np.count_nonzero((np.floor(up) != np.floor(q)) | (np.floor(down) != np.floor(q))))


def _far_voxels(rng, count, voxel):
    """`count` points in other voxels, so that the layout has bits on every axis"""
    cells = np.array([[3, 0, 1], [2, 2, 0], [5, 1, 2], [0, 3, 3], [4, 3, 1]], dtype=np.float64)
    return (cells[rng.integers(0, len(cells), count)] + rng.uniform(0.2, 0.8, size=(count, 3))) * voxel


def _interleave(rng, groups):
    """the groups' points at random places of one cloud, every group in its own order -> (xyz, every group's indices, ascending)"""
    total = sum(g.shape[0] for g in groups)
    places = rng.permutation(total)
    xyz, where, at = np.empty((total, 3), dtype=np.float32), [], 0
    for g in groups:
        idx = np.sort(places[at:at + g.shape[0]])
        xyz[idx] = g
        where.append(idx)
        at += g.shape[0]
    return xyz, where


def subnormal_cloud(count, seed):
    """voxel 1.0.  The voxel at the origin holds `count` points within a few 1e-20 of each other: their squared distances to their
    centroid are subnormal float32 numbers; the other voxels are ordinary.  -> (xyz, the origin voxel's indices, ascending)"""
    rng = np.random.default_rng(seed)
    tight = rng.integers(0, 40, size=(count, 3)).astype(np.float64) * 1e-21
    tight[rng.integers(0, count)] = 0.0                     # the minimum of the cloud
    xyz, where = _interleave(rng, [tight.astype(np.float32), _far_voxels(rng, 3 * count, 1.0).astype(np.float32)])
    return xyz, where[0]


def overflow_cloud(count, seed):
    """voxel 1e20.  The voxel at the origin holds `count` points within 5 % of its corners; the next one in x holds as many near its
    corners, in front of count // 2 near its middle.  A distance of more than about 1.85e19 along one axis squares to +inf in
    float32.  -> (xyz, the corner voxel's indices, the mixed voxel's indices), ascending"""
    rng = np.random.default_rng(seed)
    v = float(np.float32(1e20))

    def corners(m):
        u = rng.uniform(0.0, 0.05, size=(m, 3))
        return np.where(rng.integers(0, 2, size=(m, 3)) == 1, 1.0 - u, u)
    corner = corners(count)
    corner[rng.integers(0, count)] = 0.0                    # the minimum of the cloud
    mixed = np.concatenate([corners(count), 0.5 + rng.uniform(-0.04, 0.04, size=(count // 2, 3))]) + [1.0, 0.0, 0.0]
    groups = [(g * v).astype(np.float32) for g in (corner, mixed, _far_voxels(rng, 2 * count, 1.0))]
    xyz, where = _interleave(rng, groups)
    return xyz, where[0], where[1]
