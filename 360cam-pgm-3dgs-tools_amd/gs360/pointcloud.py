"""Point-cloud thinning for 3DGS training: the data-parallel part of gs360_PlyOptimizer.py on the GPU (VOX-SPEC v1 and OCT-SPEC v1,
DESIGN.md 15 and 16).

`Cloud` keeps the points resident on the device; a voxel-size probe of `voxel_downsample_to_target` then costs a key pass, a sort and
a count, and only the count comes back.  The module functions carry the reference's names, signatures, return values and printed
lines (PLY:110-128, 747-1171); the search arithmetic is Python floats on the host as there.

Keys are float32: the reference's arrays are float32 and a Python-float voxel is a weak scalar, so `(xyz - xyz_min) / voxel` is
float32 arithmetic under NumPy 2.  A voxel passed as a NumPy float64 is taken as float(voxel) and meets the same float32 grid.
A grid too fine for 64-bit packed keys (the shrink loop's 1e-9 corner) is counted and picked on the host with NumPy.

The adaptive octree sampling (PLY:1174-1407) sorts 36-bit path codes on the device, walks the split queue over counts inside the
library and picks the kept leaves on the device (`Cloud.adaptive_downsample`, `adaptive_voxel_downsample`); only max_depth=12 is built.

PLY files are read and written here (ASCII, binary little- and big-endian vertex elements; the writer's bytes are the reference's
binary little-endian x/y/z + red/green/blue file).
"""
import math
import os
import pathlib
import sys
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import capi

SKY_AXIS_CHOICES = ("+X", "-X", "+Y", "-Y", "+Z", "-Z")
SH_C0 = 0.28209479177387814
STRATEGIES = {"first": capi.VOXEL_FIRST, "center": capi.VOXEL_CENTER, "centroid": capi.VOXEL_CENTROID, "random": capi.VOXEL_SEGMENTS}


def adaptive_mode_from_env():
    """-> True when --downsample-method adaptive runs on the device.  GS360_PLY_ADAPTIVE = off (default: the flag is refused as it was
    before the octree was built) | device."""
    mode = os.environ.get("GS360_PLY_ADAPTIVE", "off")
    if mode not in ("off", "device"):
        raise ValueError(f"GS360_PLY_ADAPTIVE must be off or device (got {mode!r})")
    return mode == "device"


# ---- statistics -------------------------------------------------------------------------------------------------------------------
@dataclass
class PointCloudStats:
    count: int
    xyz_min: np.ndarray
    xyz_max: np.ndarray
    extent: np.ndarray
    volume: float


def _fmt3(a):
    return f"({float(a[0]):.6g}, {float(a[1]):.6g}, {float(a[2]):.6g})"


def _stats_from_bounds(n, xyz_min, xyz_max):
    xyz_min = np.asarray(xyz_min, dtype=np.float32)
    xyz_max = np.asarray(xyz_max, dtype=np.float32)
    extent = np.maximum(xyz_max - xyz_min, 1e-9)
    return PointCloudStats(int(n), xyz_min, xyz_max, extent, float(extent[0] * extent[1] * extent[2]))


def compute_point_cloud_stats(xyz):
    """bounding-box statistics (PLY:110-128), with NumPy on the host: the statistics-only run needs no GPU"""
    n = int(xyz.shape[0])
    if n == 0:
        zeros = np.zeros(3, dtype=np.float32)
        return PointCloudStats(0, zeros, zeros, zeros, 0.0)
    return _stats_from_bounds(n, xyz.min(axis=0), xyz.max(axis=0))


def print_point_cloud_stats(stats, include_voxel_reference=True):
    print(f"input_points={stats.count:,}")
    print(f"[aabb] min={_fmt3(stats.xyz_min)}  max={_fmt3(stats.xyz_max)}  extent={_fmt3(stats.extent)}  volume~{stats.volume:.6g}")
    if include_voxel_reference:
        v0 = (stats.volume / float(stats.count)) ** (1.0 / 3.0) if stats.volume > 0.0 and stats.count > 0 else 1e-3
        lo = max(v0 / 64.0, 1e-9)
        hi = max(v0 * 64.0, lo * 2.0)
        print(f"[init] v0~{v0:.6g}  lo={lo:.6g}  hi={hi:.6g}")


# ---- colours ----------------------------------------------------------------------------------------------------------------------
def _float_rgb_to_u8(values):
    """float colours in 0..1 or 0..255 -> uint8 (the scale is chosen by the largest finite value)"""
    v = values.astype(np.float32, copy=False)
    finite = v[np.isfinite(v)]
    if finite.size == 0:
        return np.zeros(v.shape, dtype=np.uint8)
    if float(finite.max()) <= 1.0 + 1e-6:
        scaled = np.clip(v, 0.0, 1.0) * 255.0
    else:
        scaled = np.clip(v, 0.0, 255.0)
    return np.clip(np.rint(scaled), 0, 255).astype(np.uint8)


def convert_3dgs_dc_to_rgb8(dc_rgb):
    """3DGS DC spherical-harmonic coefficients -> 8-bit RGB"""
    rgb01 = np.clip(dc_rgb.astype(np.float32, copy=False) * SH_C0 + 0.5, 0.0, 1.0)
    return np.clip(np.rint(rgb01 * 255.0), 0, 255).astype(np.uint8)


# ---- PLY --------------------------------------------------------------------------------------------------------------------------
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def _ply_header(data):
    """-> (format, [(element name, count, [(property name, type) or (name, (count type, item type))])], offset of the body)"""
    if not data.startswith(b"ply"):
        raise ValueError("not a PLY file")
    end = data.find(b"end_header")
    if end < 0:
        raise ValueError("PLY header without end_header")
    body = data.find(b"\n", end) + 1
    fmt, elements = None, []
    for line in data[:end].decode("ascii", errors="replace").splitlines():
        parts = line.split()
        if not parts or parts[0] in ("ply", "comment", "obj_info"):
            continue
        if parts[0] == "format":
            fmt = parts[1]
        elif parts[0] == "element":
            elements.append((parts[1], int(parts[2]), []))
        elif parts[0] == "property":
            if not elements:
                raise ValueError("PLY property outside an element")
            if parts[1] == "list":
                elements[-1][2].append((parts[4], (_PLY_TYPES[parts[2]], _PLY_TYPES[parts[3]])))
            else:
                if parts[1] not in _PLY_TYPES:
                    raise ValueError(f"unknown PLY property type: {parts[1]}")
                elements[-1][2].append((parts[2], _PLY_TYPES[parts[1]]))
    if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
        raise ValueError(f"unknown PLY format: {fmt}")
    return fmt, elements, body


def _read_ply_elements(path):
    """every element without list properties as a structured array, in file order: [(name, array)]"""
    data = pathlib.Path(path).read_bytes()
    fmt, elements, at = _ply_header(data)
    out = []
    if fmt == "ascii":
        lines = data[at:].decode("ascii", errors="replace").splitlines()
        lines = [ln for ln in lines if ln.strip()]
        row = 0
        for name, count, props in elements:
            rows = lines[row:row + count]
            row += count
            if any(isinstance(t, tuple) for _n, t in props):
                continue
            if len(rows) < count:
                raise ValueError(f"PLY element {name} is cut short")
            arr = np.empty(count, dtype=[(n, t) for n, t in props])
            if count:
                table = np.array([ln.split()[:len(props)] for ln in rows], dtype=np.float64).reshape(count, len(props))
                for c, (n, _t) in enumerate(props):
                    arr[n] = table[:, c]
            out.append((name, arr))
        return out
    order = "<" if fmt == "binary_little_endian" else ">"
    for name, count, props in elements:
        if any(isinstance(t, tuple) for _n, t in props):
            for _ in range(count):                         # a list element in front of the vertices: walked, not kept
                for _n, t in props:
                    if isinstance(t, tuple):
                        c = int(np.frombuffer(data, dtype=order + t[0], count=1, offset=at)[0])
                        at += np.dtype(t[0]).itemsize + c * np.dtype(t[1]).itemsize
                    else:
                        at += np.dtype(t).itemsize
            continue
        dt = np.dtype([(n, order + t) for n, t in props])
        if at + count * dt.itemsize > len(data):
            raise ValueError(f"PLY element {name} is cut short")
        out.append((name, np.frombuffer(data, dtype=dt, count=count, offset=at)))
        at += count * dt.itemsize
    return out


def _extract_xyz_rgb_from_structured(v):
    """the reference's colour-field rules (PLY:305-362): integer or float red/green/blue, r/g/b, diffuse_*, f_dc_* through SH_C0,
    else white"""
    names = v.dtype.names
    if not all(k in names for k in ("x", "y", "z")):
        raise ValueError("Could not find x, y, z fields")
    xyz = np.stack([v["x"].astype(np.float32), v["y"].astype(np.float32), v["z"].astype(np.float32)], axis=1)
    rgb = None
    for r, g, b in (("red", "green", "blue"), ("r", "g", "b"), ("diffuse_red", "diffuse_green", "diffuse_blue")):
        if r in names and g in names and b in names:
            cols = [v[r], v[g], v[b]]
            if any(c.dtype.kind == "f" for c in cols):
                rgb = _float_rgb_to_u8(np.stack(cols, axis=1))
            else:
                rgb = np.stack(cols, axis=1).astype(np.uint8, copy=False)
            break
    if rgb is None and all(c in names for c in ("f_dc_0", "f_dc_1", "f_dc_2")):
        rgb = convert_3dgs_dc_to_rgb8(np.stack([v["f_dc_0"], v["f_dc_1"], v["f_dc_2"]], axis=1))
    if rgb is None:
        rgb = np.full((xyz.shape[0], 3), 255, dtype=np.uint8)
    return xyz, rgb


def load_ply_xyz_rgb(path):
    """-> (xyz float32 n x 3, rgb uint8 n x 3) of the file's vertex element (or its first element with x, y, z)"""
    elements = _read_ply_elements(path)
    vdata = next((arr for name, arr in elements if name == "vertex"), None)
    if vdata is None:
        vdata = next((arr for _name, arr in elements if arr.dtype.names and all(k in arr.dtype.names for k in ("x", "y", "z"))), None)
    if vdata is None:
        raise ValueError(f"Could not find a vertex element with x, y, z: {path}")
    return _extract_xyz_rgb_from_structured(vdata)


def ply_binary_little_bytes(xyz, rgb):
    """the bytes of the reference's output file: float x/y/z and uchar red/green/blue, binary little-endian"""
    if xyz.shape[0] != rgb.shape[0]:
        raise ValueError("xyz and rgb must have the same number of rows")
    n = xyz.shape[0]
    arr = np.empty(n, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    for c, name in enumerate(("x", "y", "z")):
        arr[name] = xyz[:, c].astype(np.float32, copy=False)
    for c, name in enumerate(("red", "green", "blue")):
        arr[name] = rgb[:, c].astype(np.uint8, copy=False)
    header = ("ply\nformat binary_little_endian 1.0\n" + f"element vertex {n}\n" + "property float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    return header.encode("ascii") + arr.tobytes()


def save_ply_binary_little(path, xyz, rgb):
    pathlib.Path(path).write_bytes(ply_binary_little_bytes(xyz, rgb))


# ---- sky points -------------------------------------------------------------------------------------------------------------------
def _axis_direction(label):
    axes = {"X": 0, "Y": 1, "Z": 2}
    text = (label or "").upper()
    if len(text) != 2 or text[0] not in "+-" or text[1] not in axes:
        return None
    vec = np.zeros(3, dtype=np.float32)
    vec[axes[text[1]]] = 1.0 if text[0] == "+" else -1.0
    return vec / np.linalg.norm(vec)


def _rotation_matrix_from_axis(axis, angle):
    """Rodrigues' rotation about `axis`, float32"""
    axis = axis / max(np.linalg.norm(axis), 1e-6)
    x, y, z = axis
    c, s = math.cos(angle), math.sin(angle)
    C = 1.0 - c
    return np.array([[c + x * x * C, x * y * C - z * s, x * z * C + y * s],
                     [y * x * C + z * s, c + y * y * C, y * z * C - x * s],
                     [z * x * C - y * s, z * y * C + x * s, c + z * z * C]], dtype=np.float32)


def _rotation_matrix_from_vectors(source, target):
    """the rotation that turns `source` onto `target`, float32"""
    src = source / max(np.linalg.norm(source), 1e-6)
    tgt = target / max(np.linalg.norm(target), 1e-6)
    c = float(np.dot(src, tgt))
    if c > 0.9999:
        return np.eye(3, dtype=np.float32)
    if c < -0.9999:
        axis = np.array([1.0, 0.0, 0.0], dtype=np.float32)
        if abs(src[0]) > 0.9:
            axis = np.array([0.0, 1.0, 0.0], dtype=np.float32)
        axis -= axis.dot(src) * src
        axis /= max(np.linalg.norm(axis), 1e-6)
        return _rotation_matrix_from_axis(axis, math.pi)
    v = np.cross(src, tgt)
    s = np.linalg.norm(v)
    vx = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]], dtype=np.float32)
    r = np.eye(3, dtype=np.float32) + vx + (vx @ vx) * ((1.0 - c) / (s * s))
    return r.astype(np.float32)


def _sample_hemisphere_points(count, sky_percent=50.0):
    """a golden-angle spiral from the pole down to the cap that covers sky_percent of the sphere"""
    idx = np.arange(count, dtype=np.float32)
    phi = math.pi * (3.0 - math.sqrt(5.0))
    coverage = float(np.clip(sky_percent, 0.0, 100.0)) / 100.0
    z_min = 1.0 - 2.0 * coverage
    z = 1.0 - (idx / count) * (1.0 - z_min)
    radius = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    return np.stack((np.cos(phi * idx) * radius, np.sin(phi * idx) * radius, z), axis=1)


def _generate_sky_points(center, axis_vec, scale, count, color, sky_percent=50.0):
    samples = _sample_hemisphere_points(count, sky_percent=sky_percent) * float(scale)
    rot = _rotation_matrix_from_vectors(np.array([0.0, 0.0, 1.0], dtype=np.float32), axis_vec)
    world = samples @ rot.T + center
    colors = np.tile(color.astype(np.uint8, copy=False), (world.shape[0], 1))
    return world.astype(np.float32, copy=False), colors


def _parse_sky_color(text):
    default = np.array([135, 206, 250], dtype=np.uint8)
    value = (text or "").strip()
    if not value:
        return default
    if "," in value:
        parts = [p.strip() for p in value.split(",")]
        if len(parts) != 3:
            raise ValueError("expected R,G,B components")
        comps = [int(float(p)) for p in parts]
    elif value.startswith("#"):
        hexval = value[1:]
        if len(hexval) == 3:
            hexval = "".join(ch * 2 for ch in hexval)
        if len(hexval) != 6:
            raise ValueError("hex color must be #RGB or #RRGGBB")
        comps = [int(hexval[i:i + 2], 16) for i in (0, 2, 4)]
    else:
        raise ValueError("use #RRGGBB or R,G,B format")
    return np.array([max(0, min(255, int(c))) for c in comps], dtype=np.uint8)


# ---- the host path of a grid too fine for packed keys -----------------------------------------------------------------------------
def _host_keys(xyz, voxel, xyz_min):
    with np.errstate(all="ignore"):
        return np.floor((xyz - np.asarray(xyz_min, dtype=np.float32).reshape(1, 3)) / voxel).astype(np.int64, copy=False)


def _host_unique_count(xyz, voxel, xyz_min):
    return int(np.unique(_host_keys(xyz, voxel, xyz_min), axis=0).shape[0])


def _host_segments(xyz, voxel, xyz_min):
    """-> (voxel keys k x 3 in lexicographic order, the indices in stable key order, the segment starts)"""
    uniq, inv = np.unique(_host_keys(xyz, voxel, xyz_min), axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    order = np.argsort(inv, kind="stable")
    starts = np.flatnonzero(np.r_[True, np.diff(inv[order]) != 0])
    return uniq, order.astype(np.int64), starts.astype(np.int64)


def _host_pick(xyz, voxel, xyz_min, representative):
    """VOX-SPEC's pick with NumPy: used where the device refuses the grid"""
    uniq, order, starts = _host_segments(xyz, voxel, xyz_min)
    if representative == "first":
        return order[starts]
    n, k = xyz.shape[0], starts.size
    lens = np.diff(np.r_[starts, n])
    gid = np.repeat(np.arange(k), lens)
    if representative == "center":
        targets = (np.asarray(xyz_min, dtype=np.float32).reshape(1, 3) + (uniq.astype(np.float32) + np.float32(0.5)) * voxel).astype(np.float32)
    else:
        sums = np.zeros((k, 3), dtype=np.float64)
        np.add.at(sums, gid, xyz[order].astype(np.float64))
        targets = (sums / lens[:, None]).astype(np.float32)
    with np.errstate(all="ignore"):
        d = xyz[order] - targets[gid]
        dist2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    low = np.minimum.reduceat(dist2, starts)
    hits = np.flatnonzero(dist2 == low[gid])
    _g, first = np.unique(gid[hits], return_index=True)
    return order[hits[first]]


def _random_pick(order, starts, lens):
    """one member of every segment (its start and length in `order`) at an offset drawn from an unseeded generator, as the reference
    draws"""
    return order[starts + np.random.default_rng().integers(lens)]


# ---- the resident cloud -----------------------------------------------------------------------------------------------------------
class Cloud:
    """n x 3 float32 points uploaded once; bounds, counts and picks run on the device against them (slot `slot` of `ctx`)."""

    def __init__(self, ctx, xyz, slot=0):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        if xyz.ndim != 2 or xyz.shape[1] != 3 or xyz.shape[0] < 1:
            raise ValueError("a cloud is an n x 3 array of at least one point")
        if xyz.shape[0] > capi.VOXEL_MAX_POINTS:
            raise capi.Gs360Error(capi.ERR_UNSUPPORTED, "a cloud of 2^31 or more points is not built")
        self.ctx, self.slot, self.xyz, self.n = ctx, slot, xyz, int(xyz.shape[0])
        self._bufs = []
        try:
            self.d_xyz = self._alloc(xyz.nbytes)
            ctx.upload(self.d_xyz, xyz, slot)
            self.scratch = self._alloc(ctx.voxel_scratch(self.n))
            self._out = self._octree = None
            self.minmax = ctx.cloud_bounds_dev(self.d_xyz, self.n, self.scratch, slot)
        except Exception:
            self.close()
            raise

    def _alloc(self, nbytes):
        buf = self.ctx.alloc(nbytes)
        self._bufs.append(buf)
        return buf

    def close(self):
        for buf in self._bufs:
            self.ctx.free(buf)
        self._bufs = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def stats(self):
        return _stats_from_bounds(self.n, self.minmax[:3], self.minmax[3:])

    def unique_count(self, voxel):
        """the number of occupied voxels of edge `voxel` (PLY:846-862)"""
        voxel = float(voxel)
        if voxel <= 0:
            raise ValueError("voxel must be > 0")
        try:
            return self.ctx.voxel_count_dev(self.d_xyz, self.n, self.minmax, voxel, self.scratch, self.slot)
        except capi.Gs360Error as exc:
            if exc.code != capi.ERR_UNSUPPORTED:
                raise
            return _host_unique_count(self.xyz, voxel, self.minmax[:3])

    def downsample_by_size(self, voxel, representative="centroid", return_indices=True):
        """the pick index of every occupied voxel, in key order, as int64 (PLY:747-843); return_indices=False: the points picked"""
        voxel = float(voxel)
        if voxel <= 0:
            raise ValueError("voxel must be > 0")
        if representative not in STRATEGIES:
            raise ValueError(f"Unknown representative strategy: {representative}")
        if self._out is None:
            self._out = [self._alloc(4 * self.n) for _ in range(3)]
        pick, order, starts = self._out
        try:
            if representative == "random":
                k = self.ctx.voxel_pick_dev(self.d_xyz, self.n, self.minmax, voxel, capi.VOXEL_SEGMENTS, self.scratch, None, order, starts, self.slot)
                starts_h = self.ctx.download(starts, (k,), np.uint32, self.slot).astype(np.int64)
                idx = _random_pick(self.ctx.download(order, (self.n,), np.uint32, self.slot).astype(np.int64), starts_h, np.diff(np.r_[starts_h, self.n]))
            else:
                k = self.ctx.voxel_pick_dev(self.d_xyz, self.n, self.minmax, voxel, STRATEGIES[representative], self.scratch, pick, None, None, self.slot)
                idx = self.ctx.download(pick, (k,), np.uint32, self.slot).astype(np.int64)
        except capi.Gs360Error as exc:
            if exc.code != capi.ERR_UNSUPPORTED:
                raise
            if representative == "random":
                _uniq, order_h, starts_h = _host_segments(self.xyz, voxel, self.minmax[:3])
                idx = _random_pick(order_h, starts_h, np.diff(np.r_[starts_h, self.n]))
            else:
                idx = _host_pick(self.xyz, voxel, self.minmax[:3], representative)
        return idx if return_indices else self.xyz[idx]

    def adaptive_downsample(self, target, weight_power=1.0, min_voxel_size=None, representative="centroid", stats=None):
        """the pick index of every kept octree leaf, in the reference's output order, as int64 (PLY:1174-1407, max_depth 12); `stats`:
        the statistics the cube is taken from, when they are not the cloud's own"""
        n = self.n
        target = n if target is None or target <= 0 else int(max(1, min(n, target)))
        if target >= n:
            return np.arange(n, dtype=np.int64)
        if representative not in STRATEGIES:
            raise ValueError(f"Unknown representative strategy: {representative}")
        if stats is None or stats.count != n:
            stats = self.stats()
        extent = np.asarray(stats.extent, dtype=np.float32)
        cube_size = float(np.max(extent))
        pad = np.maximum((cube_size - extent) * 0.5, 0.0)
        cube_min = np.asarray(stats.xyz_min - pad, dtype=np.float32)
        min_voxel = float(min_voxel_size) if min_voxel_size else 0.0
        power = float(weight_power) if weight_power is not None else 1.0
        if self._octree is None:
            self._octree = (self._alloc(self.ctx.octree_scratch(n)), self._alloc(4 * n))
        scratch, order = self._octree
        picks, starts, counts, _ms = self.ctx.octree_pick_dev(self.d_xyz, n, cube_min, cube_size, target, power, min_voxel, STRATEGIES[representative],
                                                              scratch, order if representative == "random" else None, self.slot)
        if representative != "random":
            return picks.astype(np.int64)
        return _random_pick(self.ctx.download(order, (n,), np.uint32, self.slot).astype(np.int64), starts.astype(np.int64), counts.astype(np.int64))


_default_ctx = None


def default_context():
    """the context the module functions use when they are not given a cloud: device 0, one slot, made on first use"""
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = capi.Context(device=0, n_slots=1)
    return _default_ctx


def close_default_context():
    global _default_ctx
    if _default_ctx is not None:
        _default_ctx.close()
        _default_ctx = None


class _Resident:
    """the caller's cloud, or one made for the call and closed after it"""

    def __init__(self, xyz, cloud):
        self.cloud, self.own = cloud, None
        if cloud is None:
            self.cloud = self.own = Cloud(default_context(), xyz)
        elif cloud.n != xyz.shape[0]:
            raise ValueError("the resident cloud is not this array")

    def __enter__(self):
        return self.cloud

    def __exit__(self, *exc):
        if self.own is not None:
            self.own.close()


def _passthrough(xyz, rgb, indices, return_indices):
    out_xyz = xyz.astype(np.float32, copy=False)
    out_rgb = rgb.astype(np.uint8, copy=False)
    return (out_xyz, out_rgb, indices) if return_indices else (out_xyz, out_rgb)


# ---- the drop-in functions --------------------------------------------------------------------------------------------------------
def voxel_downsample_by_size(xyz, rgb, voxel, *, representative="centroid", return_indices=False, cloud=None):
    """one point per occupied voxel of edge `voxel` (PLY:747-843); `cloud`: the resident Cloud of `xyz`, when the caller keeps one"""
    if xyz.shape[0] == 0:
        return _passthrough(xyz, rgb, np.zeros((0,), dtype=np.int64), return_indices)
    with _Resident(xyz, cloud) as res:
        pick_idx = res.downsample_by_size(voxel, representative, return_indices=True)
    return _passthrough(xyz[pick_idx], rgb[pick_idx], pick_idx, return_indices)


def voxel_downsample_to_target(xyz, rgb, target_points, tol_ratio=0.02, max_iter=32, stats: Optional[PointCloudStats] = None,
                               log_bounds=True, representative="centroid", return_indices=False, *, cloud=None):
    """the voxel-size search towards `target_points` (PLY:865-1030): the same memoised probes, steps and log lines; every probe is a
    device count on the resident cloud"""
    n = xyz.shape[0]
    if n == 0:
        return _passthrough(xyz, rgb, np.zeros((0,), dtype=np.int64), return_indices)
    if target_points <= 0 or target_points >= n:           # no probe, no device
        print(f"[target] input_points={n:,}  target={target_points:,}  tol=+/-{tol_ratio * 100:.1f}%  max_iter={max_iter}")
        print(f"[target] skip: target={target_points} is out of range (output = input)")
        return _passthrough(xyz, rgb, np.arange(n, dtype=np.int64), return_indices)
    with _Resident(xyz, cloud) as res:
        if stats is None or stats.count != n:
            stats = res.stats()
        print(f"[target] input_points={n:,}  target={target_points:,}  tol=+/-{tol_ratio * 100:.1f}%  max_iter={max_iter}")
        vol = stats.volume
        v0 = (vol / float(target_points)) ** (1.0 / 3.0) if vol > 0 else 1e-3
        cache = {}

        def count(voxel_size):
            key = round(float(voxel_size), 12)
            if key not in cache:
                cache[key] = res.unique_count(voxel_size)
            return cache[key]

        min_voxel = 1e-9
        lo = max(v0 / 64.0, min_voxel)
        hi = max(v0 * 64.0, lo * 2.0)
        cnt_lo = count(lo)
        if cnt_lo < target_points:
            print(f"[shrink] initial lo={lo:.6g} -> unique={cnt_lo:,} (below target); shrinking lower bound")
            step = 0
            while cnt_lo < target_points and lo > min_voxel:
                halved = max(lo * 0.5, min_voxel)
                if halved == lo:
                    break
                lo = halved
                cnt_lo = count(lo)
                step += 1
                print(f"[shrink {step:02d}] lo={lo:.6g} -> unique={cnt_lo:,}")
                if step >= 32:
                    break
            if cnt_lo < target_points:
                print("[shrink] warning: minimum voxel size still below target; will use best available count.")
        hi = max(hi, lo * 2.0)
        if log_bounds:
            print(f"[aabb] min={_fmt3(stats.xyz_min)}  max={_fmt3(stats.xyz_max)}  extent={_fmt3(stats.extent)}  volume~{vol:.6g}")
        print(f"[init] v0~{v0:.6g}  lo={lo:.6g}  hi={hi:.6g}")
        for _ in range(10):
            cnt_hi = count(hi)
            print(f"[expand] try hi={hi:.6g} -> unique={cnt_hi:,}")
            if cnt_hi <= target_points:
                break
            hi *= 2.0
        else:
            print("[expand] warning: could not find a sufficient upper bound")
        best_voxel, best_diff, best_cnt = v0, 10 ** 18, n
        for it in range(1, max_iter + 1):
            mid = 0.5 * (lo + hi)
            cnt = count(mid)
            diff = abs(cnt - target_points)
            if diff < best_diff:
                best_diff, best_voxel, best_cnt = diff, mid, cnt
            print(f"[iter {it:02d}] voxel={mid:.2f}  unique={cnt:,}")
            if diff / float(target_points) <= tol_ratio:
                print(f"[stop] within tolerance: voxel={mid:.6g}  unique={cnt:,}")
                best_voxel, best_cnt = mid, cnt
                break
            if cnt > target_points:
                lo = mid
            else:
                hi = mid
        print(f"[best] voxel~{best_voxel:.6g}  unique~{best_cnt:,}  (best_diff={best_diff:,})")
        result = voxel_downsample_by_size(xyz, rgb, best_voxel, representative=representative, return_indices=True, cloud=res)
    print(f"[final] voxel={best_voxel:.6g}  out_points={result[0].shape[0]:,}")
    return result if return_indices else result[:2]


def spatial_hash_downsample_one_pass(xyz, rgb, target_points=None, voxel_size=None, stats: Optional[PointCloudStats] = None,
                                     representative="centroid", return_indices=False, *, cloud=None):
    """one voxel pass at a given or estimated size, the estimate corrected by at most three probes (PLY:1033-1171)"""
    n = int(xyz.shape[0])
    if n == 0:
        return _passthrough(xyz, rgb, np.zeros((0,), dtype=np.int64), return_indices)
    everything = np.arange(n, dtype=np.int64)
    if voxel_size is not None and voxel_size > 0:
        voxel = float(voxel_size)
        print(f"[spatial-hash] fixed voxel-size={voxel:.6g}")
        result = voxel_downsample_by_size(xyz, rgb, voxel, representative=representative, return_indices=True, cloud=cloud)
    elif target_points is not None and target_points > 0:
        target = int(max(1, min(n, target_points)))
        if target >= n:
            print(f"[spatial-hash] skip: target={target:,} is not smaller than input={n:,}")
            return _passthrough(xyz, rgb, everything, return_indices)
        with _Resident(xyz, cloud) as res:
            if stats is None or stats.count != n:
                stats = res.stats()
            vol = stats.volume
            voxel = max(float((vol / float(target)) ** (1.0 / 3.0) if vol > 0 else 1e-3), 1e-9)
            probes = []
            prev_voxel = prev_count = None
            max_probes = 3
            for probe in range(1, max_probes + 1):
                cnt = res.unique_count(voxel)
                probes.append((probe, voxel, cnt))
                if cnt <= 0:
                    break
                ratio = float(cnt) / float(target)
                if abs(ratio - 1.0) <= 0.06 or probe >= max_probes:
                    break
                if prev_voxel is not None and prev_count is not None and prev_count > 0 and cnt != prev_count and abs(voxel - prev_voxel) > 1e-12:
                    try:
                        dim = math.log(float(cnt) / float(prev_count)) / math.log(float(prev_voxel) / float(voxel))
                    except (ValueError, ZeroDivisionError):
                        dim = 2.0
                    if not np.isfinite(dim):
                        dim = 2.0
                    dim = max(1.2, min(3.0, abs(float(dim))))
                else:
                    dim = 1.45 if ratio < 0.2 else 1.7 if ratio < 0.5 else 2.6 if ratio > 2.0 else 2.1
                scale = min(2.8, max(0.12, ratio ** (1.0 / dim)))
                new_voxel = max(voxel * scale, 1e-9)
                prev_voxel, prev_count = voxel, cnt
                if abs(new_voxel - voxel) <= max(1e-9, voxel * 1e-4):
                    break
                voxel = new_voxel
            for probe, probe_voxel, probe_count in probes:
                print(f"[spatial-hash probe {probe}] voxel={probe_voxel:.6g} unique={probe_count:,}")
            print(f"[spatial-hash] target~{target:,} -> voxel={voxel:.6g} probes={len(probes)}")
            result = voxel_downsample_by_size(xyz, rgb, voxel, representative=representative, return_indices=True, cloud=res)
    else:
        print("[spatial-hash] skip (no voxel-size/target-points)")
        return _passthrough(xyz, rgb, everything, return_indices)
    print(f"[spatial-hash] voxel={voxel:.6g}  out_points={result[0].shape[0]:,} (approx)")
    return result if return_indices else result[:2]


def adaptive_voxel_downsample(xyz, rgb, target_points, weight_power=1.0, stats: Optional[PointCloudStats] = None, min_voxel_size=None,
                              representative="centroid", max_depth=12, return_indices=False, *, cloud=None):
    """the adaptive octree sampling that keeps detail where the cloud is dense (PLY:1174-1407): the reference's leaves and picks,
    index for index; the tree is built to the reference's default depth of 12 only"""
    n = int(xyz.shape[0])
    if n == 0:
        return _passthrough(xyz, rgb, np.zeros((0,), dtype=np.int64), return_indices)
    target = n if target_points is None or target_points <= 0 else int(max(1, min(n, target_points)))
    if target >= n:                                        # no tree, no device
        return _passthrough(xyz, rgb, np.arange(n, dtype=np.int64), return_indices)
    if max_depth != 12:
        raise capi.Gs360Error(capi.ERR_UNSUPPORTED, f"an octree of max_depth={max_depth} is not built: path codes hold 12 levels")
    with _Resident(xyz, cloud) as res:
        pick_idx = res.adaptive_downsample(target, weight_power, min_voxel_size, representative, stats=stats)
    return _passthrough(xyz[pick_idx], rgb[pick_idx], pick_idx, return_indices)
