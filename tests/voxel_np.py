"""VOX-SPEC v1 in NumPy: the packed-key stable-sort restatement of gs360_PlyOptimizer.py's
compute_point_cloud_stats, _unique_voxel_count and voxel_downsample_by_size.  The project's own code; the device kernels
(csrc/gs360_voxel.hip) are compared with it bit for bit, and it is compared with the reference's recorded picks
(tests/golden/plyopt_goldens.npz)."""
import numpy as np

TWO63 = np.float32(9223372036854775808.0)


def bounds(xyz):
    """-> float32[6]: the per-axis minimum, then the maximum"""
    xyz = np.asarray(xyz, dtype=np.float32)
    return np.concatenate([xyz.min(axis=0), xyz.max(axis=0)]).astype(np.float32)


def axis_keys(xyz, lo, voxel):
    """k_a = (int64) floorf((x_a - min_a) / (float) voxel): one float32 subtract, one float32 divide"""
    v = np.float32(voxel)
    with np.errstate(all="ignore"):
        q = np.floor((np.asarray(xyz, dtype=np.float32) - np.asarray(lo, dtype=np.float32).reshape(1, 3)) / v)
    assert q.dtype == np.float32
    return q


def layout(minmax, voxel):
    """the bit lengths (b_x, b_y, b_z) of the largest keys, from the cloud's maximum by the points' own expression; None when a key
    needs more than 63 bits or the three more than 64 (the host path)"""
    v = np.float32(voxel)
    if not (np.isfinite(v) and v > 0):
        return None
    q = axis_keys(np.asarray(minmax[3:], dtype=np.float32).reshape(1, 3), minmax[:3], voxel)[0]
    if not np.all((q >= 0) & (q < TWO63)):
        return None
    bits = [int(int(k).bit_length()) for k in q.astype(np.int64)]
    return bits if sum(bits) <= 64 else None


def packed_keys(xyz, minmax, voxel):
    """-> uint64 keys, x most significant; None where layout() is"""
    bits = layout(minmax, voxel)
    if bits is None:
        return None
    k = axis_keys(xyz, minmax[:3], voxel).astype(np.int64).astype(np.uint64)
    sx, sy = np.uint64(bits[1] + bits[2]), np.uint64(bits[2])
    kx = k[:, 0] << sx if bits[1] + bits[2] < 64 else np.zeros_like(k[:, 0])
    return kx | (k[:, 1] << sy) | k[:, 2]


def triple_keys(xyz, minmax, voxel):
    with np.errstate(all="ignore"):
        return axis_keys(xyz, minmax[:3], voxel).astype(np.int64)


def unique_count(xyz, voxel, minmax=None):
    """(count, whether the packed path was taken)"""
    xyz = np.asarray(xyz, dtype=np.float32)
    minmax = bounds(xyz) if minmax is None else minmax
    keys = packed_keys(xyz, minmax, voxel)
    if keys is None:
        return int(np.unique(triple_keys(xyz, minmax, voxel), axis=0).shape[0]), False
    return int(np.unique(keys).shape[0]), True


def segments(xyz, voxel, minmax=None):
    """-> (sorted packed keys, the indices in stable key order, the segment starts, the bit lengths)"""
    xyz = np.asarray(xyz, dtype=np.float32)
    minmax = bounds(xyz) if minmax is None else minmax
    keys = packed_keys(xyz, minmax, voxel)
    assert keys is not None, "the grid is too fine for packed keys"
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    return ks, order.astype(np.int64), starts.astype(np.int64), layout(minmax, voxel)


def pick(xyz, voxel, representative, minmax=None):
    """the pick index per voxel, in key order (int64)"""
    xyz = np.asarray(xyz, dtype=np.float32)
    minmax = bounds(xyz) if minmax is None else minmax
    if representative == "first":
        _ks, order, starts, _bits = segments(xyz, voxel, minmax)
        return order[starts]
    order, starts, gid, dist2 = distances(xyz, voxel, representative, minmax)
    low = np.minimum.reduceat(dist2, starts)
    hits = np.flatnonzero(dist2 == low[gid])               # the first minimum of every segment
    _g, first = np.unique(gid[hits], return_index=True)
    return order[hits[first]]


def distances(xyz, voxel, representative, minmax=None):
    """-> (the indices in stable key order, the segment starts, the segment of every sorted position, its float32 squared distance
    to its voxel's `center` or `centroid`)"""
    xyz = np.asarray(xyz, dtype=np.float32)
    minmax = bounds(xyz) if minmax is None else minmax
    ks, order, starts, bits = segments(xyz, voxel, minmax)
    n, k = xyz.shape[0], starts.size
    lens = np.diff(np.r_[starts, n])
    gid = np.repeat(np.arange(k), lens)
    v = np.float32(voxel)
    if representative == "center":
        head = ks[starts]
        mask = lambda b: np.uint64((1 << b) - 1)
        kx = head >> np.uint64(bits[1] + bits[2]) if bits[1] + bits[2] < 64 else np.zeros_like(head)
        kk = np.stack([kx, (head >> np.uint64(bits[2])) & mask(bits[1]), head & mask(bits[2])], axis=1)
        targets = np.asarray(minmax[:3], dtype=np.float32).reshape(1, 3) + (kk.astype(np.float32) + np.float32(0.5)) * v
    elif representative == "centroid":
        sums = np.zeros((k, 3), dtype=np.float64)
        np.add.at(sums, gid, xyz[order].astype(np.float64))   # one by one, in segment order
        targets = (sums / lens[:, None].astype(np.float64)).astype(np.float32)
    else:
        raise ValueError(representative)
    assert targets.dtype == np.float32
    with np.errstate(all="ignore"):
        d = xyz[order] - targets[gid]
        dist2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert dist2.dtype == np.float32
    return order, starts, gid, dist2


def downsample_ply_bytes(xyz, rgb, idx):
    """the bytes of the reference's output file for the points `idx`"""
    from gs360 import pointcloud
    return pointcloud.ply_binary_little_bytes(xyz[idx], rgb[idx])
