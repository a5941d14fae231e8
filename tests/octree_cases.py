"""Clouds at the edges of OCT-SPEC v1, shared by the host check and the GPU test: each entry is
(name, xyz float32, [(target, weight power, smallest voxel or None)]); every entry is run with `centroid`, `center` and `first`."""
import numpy as np

import octree_np

STRATEGIES = ("centroid", "center", "first")


def plane_cloud():
    """a cube of edge 64 at the origin: points exactly on centre planes k * 64 / 4096 of every level, their neighbours one ulp below,
    and both corners of the cube (the maximum corner's code is all ones)"""
    rng = np.random.default_rng(4096)
    k = np.concatenate([rng.integers(1, 4096, size=(300, 3)), [[2048, 2048, 2048], [1024, 3072, 512], [1, 4095, 2047]]])
    on = (k / 64.0).astype(np.float32)
    below = np.nextafter(on, np.float32(-np.inf))
    mixed = np.where(rng.integers(0, 2, size=on.shape).astype(bool), on, below)
    return np.concatenate([on, below, mixed, [[0.0, 0.0, 0.0], [64.0, 64.0, 64.0]]]).astype(np.float32)


def cluster_cloud(sizes=(30, 31, 33, 63, 64, 65)):
    """one tight cluster per octant of the root (the first two also hold a corner of the cube: leaves of 31, 32, 33, 63, 64 and 65
    points): at a target of len(sizes) every cluster is one leaf"""
    rng = np.random.default_rng(3233)
    corners = [(-1, -1, -1), (1, 1, 1), (-1, 1, -1), (1, -1, 1), (-1, -1, 1), (1, 1, -1)]
    parts = [np.array(c) * 10.0 + rng.uniform(-0.5, 0.5, size=(m, 3)) for c, m in zip(corners, sizes)]
    pts = np.concatenate(parts + [[[-10.5, -10.5, -10.5], [10.5, 10.5, 10.5]]]).astype(np.float32)
    return pts[rng.permutation(pts.shape[0])]


def tied_cloud():
    """the eight corners of a cube, twice: every point is as far from the root's centroid and centre as any other"""
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float32)
    return np.concatenate([corners[::-1], corners])


def cases():
    rng = np.random.default_rng(1616)
    out = [("two points", np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]], np.float32), [(1, 1.0, None)]),
           ("identical points", np.tile(np.array([[1.5, -2.0, 0.25]], np.float32), (50, 1)), [(1, 1.0, None), (5, 1.0, None), (49, 0.0, None)])]
    dup = np.repeat(rng.normal(size=(30, 3)), 5, axis=0).astype(np.float32)
    out.append(("five-fold duplicates", dup[rng.permutation(150)], [(29, 1.0, None), (31, 1.0, None), (149, 1.0, None), (149, 0.0, None)]))
    out.append(("centre planes", plane_cloud(), [(7, 1.0, None), (200, 1.0, None), (600, 2.0, None), (910, 0.0, None)]))
    thin = (rng.uniform(-1.0, 0.0, size=(700, 3)) * np.array([1000.0, 1.0, 0.001]) - np.array([5.0, 300.0, 0.0])).astype(np.float32)
    out.append(("negative, 1000 : 1 : 0.001", thin, [(8, 1.0, None), (90, 1.5, None), (650, 0.5, None)]))
    out.append(("leaf lengths around 32 and 64", cluster_cloud(), [(6, 1.0, None), (8, 1.0, None)]))
    out.append(("all distances tied", tied_cloud(), [(1, 1.0, None), (2, 1.0, None)]))
    gauss = (rng.normal(size=(1200, 3)) * np.array([3.0, 2.0, 1.0])).astype(np.float32)
    _m, cube_size = octree_np.cube(gauss)
    out.append(("targets 7, 8, 9 and the weights", gauss, [(t, w, None) for t in (7, 8, 9) for w in (0.0, 0.5, 1.5, 2.0, -1.0)]))
    out.append(("smallest voxels", gauss, [(300, 1.0, cube_size), (300, 1.0, cube_size * 2.0), (300, 1.0, cube_size / 8.0), (300, 0.0, cube_size / 8.0)]))
    return out
