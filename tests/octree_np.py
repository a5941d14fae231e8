"""OCT-SPEC v1 restated with NumPy: the adaptive octree sampling of gs360_PlyOptimizer.py (PLY:1174-1407) as one
stable sort of 36-bit path codes, a heap over ranges of the sorted array that looks at counts only, and a pick per leaf over its
points in ascending original index.  tests/test_octree_cpu.py holds it to the unmodified reference's index arrays
(tests/golden/octree_goldens.npz); the device and the host check are held to it."""
import heapq

import numpy as np

DEPTH = 12
EPS = 1e-9


def cube(xyz):
    """-> (cube_min float32[3], cube_size float): the padded cube of the cloud's bounding box (PLY:1231-1242)"""
    xyz_min, xyz_max = xyz.min(axis=0).astype(np.float32), xyz.max(axis=0).astype(np.float32)
    extent = np.maximum(xyz_max - xyz_min, 1e-9)
    cube_size = float(np.max(extent))
    pad = np.maximum((cube_size - extent) * 0.5, 0.0)
    return np.asarray(xyz_min - pad, dtype=np.float32), cube_size


def halves(cube_size):
    """(float) (size_l * 0.5) for l = 0..12: the step of the corner's add chain at every level"""
    return np.array([cube_size * 0.5 ** l * 0.5 for l in range(DEPTH + 1)], dtype=np.float32)


def descend(xyz, cube_min, cube_size, depth=DEPTH):
    """the add chain over `depth` levels -> (codes uint64, corners float32 n x 3)"""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    m = np.tile(np.asarray(cube_min, dtype=np.float32), (xyz.shape[0], 1))
    code = np.zeros(xyz.shape[0], dtype=np.uint64)
    for h in halves(cube_size)[:depth]:
        c = m + h
        bit = xyz >= c
        m = np.where(bit, c, m)
        child = (bit[:, 0].astype(np.uint64) << np.uint64(2)) | (bit[:, 1].astype(np.uint64) << np.uint64(1)) | bit[:, 2].astype(np.uint64)
        code = (code << np.uint64(3)) | child
    return code, m


def codes(xyz, cube_min, cube_size):
    return descend(xyz, cube_min, cube_size)[0]


def levels(sorted_codes):
    """per sorted position the first level (1..12) at which its code differs from its predecessor's, 13 if equal; position 0 holds 0"""
    lvl = np.full(sorted_codes.shape[0], DEPTH + 1, dtype=np.uint8)
    diff = sorted_codes[1:] ^ sorted_codes[:-1]
    for level in range(DEPTH, 0, -1):
        lvl[1:][(diff >> np.uint64(3 * (DEPTH - level))) != 0] = level
    lvl[0] = 0
    return lvl


def weight_of(count, power):
    power = max(float(power), 0.0)
    return 1.0 if power == 0.0 else float(count) ** power


def walk(lvl, target, power=1.0, min_voxel=None, cube_size=1.0):
    """the split loop over ranges of the sorted array -> [(start, end, depth)] of every leaf, in the order the loop made them"""
    n = lvl.shape[0]
    heap, leaves, seq = [(-weight_of(n, power), 0, 0, n, 0)], [], 1
    while heap and len(leaves) + len(heap) < target:
        _w, _s, s, e, d = heapq.heappop(heap)
        size = cube_size * 0.5 ** d
        if e - s <= 1 or d >= DEPTH or (min_voxel and size <= min_voxel + EPS) or size * 0.5 <= EPS:
            leaves.append((s, e, d))
            continue
        cuts = np.r_[s, s + 1 + np.flatnonzero(lvl[s + 1:e] <= d + 1), e]
        for a, b in zip(cuts[:-1].tolist(), cuts[1:].tolist()):
            if b - a == 1:
                leaves.append((a, b, d + 1))
            else:
                heapq.heappush(heap, (-weight_of(b - a, power), seq, a, b, d + 1))
                seq += 1
        if len(leaves) + len(heap) >= target:
            break
    return leaves + [(s, e, d) for _w, _s, s, e, d in heap]


def select(leaves, order, target, power=1.0):
    """the leaves kept, in output order: weight and count descending, then the smallest original index ascending"""
    keyed = sorted(leaves, key=lambda lf: (-weight_of(lf[1] - lf[0], power), -(lf[1] - lf[0]), int(order[lf[0]:lf[1]].min())))
    return keyed[:min(len(keyed), target)]


def centres(xyz, segs, cube_min, cube_size):
    """the centre of every leaf of `segs`: its corner, re-accumulated from its first point's path, plus the half of its size"""
    heads, depths = np.array([idx[0] for idx, _d in segs]), np.array([d for _idx, d in segs])
    out = np.empty((len(segs), 3), dtype=np.float32)
    for d in np.unique(depths):
        out[depths == d] = descend(xyz[heads[depths == d]], cube_min, cube_size, int(d))[1] + halves(cube_size)[d]
    return out


def pick_leaf(xyz, idx, how, centre):
    """idx: the leaf's points in ascending original index; centre: the leaf's (for `center`)"""
    if how == "first" or idx.shape[0] == 1:
        return int(idx[0])
    pts = xyz[idx]
    if how == "center":
        t = centre
    else:
        t = np.cumsum(pts, axis=0, dtype=np.float32)[-1] / np.float32(idx.shape[0])      # one by one, in index order
    d = pts - t
    dist2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return int(idx[int(np.argmin(dist2))])


def segments(xyz, target, power=1.0, min_voxel=None):
    """-> [(the leaf's indices ascending, depth)] of the kept leaves in output order, cube_min, cube_size"""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    cube_min, cube_size = cube(xyz)
    code = codes(xyz, cube_min, cube_size)
    order = np.argsort(code, kind="stable")
    leaves = walk(levels(code[order]), target, power, min_voxel, cube_size)
    kept = select(leaves, order, target, power)
    return [(np.sort(order[s:e]), d) for s, e, d in kept], cube_min, cube_size


def pick(xyz, target, power=1.0, min_voxel=None, how="centroid"):
    """adaptive_voxel_downsample(..., return_indices=True)[2] for 0 < target < n"""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    segs, cube_min, cube_size = segments(xyz, target, power, min_voxel)
    mid = centres(xyz, segs, cube_min, cube_size)
    return np.array([pick_leaf(xyz, idx, how, mid[j]) for j, (idx, _d) in enumerate(segs)], dtype=np.int64)
