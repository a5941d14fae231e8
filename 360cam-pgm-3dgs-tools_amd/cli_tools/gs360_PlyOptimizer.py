#!/usr/bin/env python3
"""gs360_PlyOptimizer -- the reference's PointCloudOptimizer with its voxel downsampling on the GPU (VOX-SPEC v1, OCT-SPEC v1).

Thins a photogrammetry point cloud before 3DGS training: loads a PLY file, keeps one point per voxel (a fixed voxel size, or a size
searched for a target count), appends further PLY files and a synthetic sky dome, and writes a binary little-endian PLY.  It keeps
the reference's flags and defaults, parser complaints, log lines and exit codes (PLY:1413-1831).  The cloud is uploaded once;
every probe of the target search is a key pass, a sort and a count on the device (gs360/pointcloud.py).  Without --out the run
prints the statistics with NumPy and needs no GPU.

--downsample-method adaptive / --adaptive (the octree sampling, PLY:1174-1407 and 1657-1703) runs when the environment says
GS360_PLY_ADAPTIVE=device: path codes, sorts and picks on the device, the split queue over counts inside the library; --voxel-size
is then the smallest voxel.  Without the variable the flag is refused with one [ERR] line before anything is written, as it was
before the octree was built.  Not built, and refused the same way: a COLMAP text-model folder as input.
"""
import argparse
import os
import sys
from pathlib import Path

_PKG = Path(__file__).resolve().parent.parent
if str(_PKG) not in sys.path:
    sys.path.insert(0, str(_PKG))

SKY_AXIS_CHOICES = ("+X", "-X", "+Y", "-Y", "+Z", "-Z")


def create_arg_parser():
    ap = argparse.ArgumentParser(prog="PointCloudOptimizer",
                                 description="Thin a point cloud for 3DGS training on the GPU (PLY in, PLY out; voxel downsampling, append, sky dome)")
    ap.add_argument("-i", "--in", dest="input", required=True, help="the PLY file to read (a COLMAP text-model folder is not built)")
    ap.add_argument("-o", "--out", dest="output", default=None, help="the PLY file to write; without it the run only prints the cloud's statistics")
    ap.add_argument("-t", "--target-points", type=int, default=None, help="about how many points to keep; goes before --voxel-size")
    ap.add_argument("-r", "--target-percent", type=float, default=None, help="the points to keep in percent of the input; becomes --target-points after loading")
    ap.add_argument("-v", "--voxel-size", type=float, default=None, help="a fixed voxel edge in the cloud's units; with the octree sampling the smallest voxel")
    ap.add_argument("--downsample-method", choices=("voxel", "spatial-hash", "adaptive"), default="voxel",
                    help="voxel: fixed size or a search for the target; spatial-hash: one pass at an estimated size; adaptive: octree sampling "
                         "that keeps detail where the cloud is dense (runs with GS360_PLY_ADAPTIVE=device in the environment, else ends with [ERR])")
    ap.add_argument("--adaptive", action="store_true", help="deprecated: the same as --downsample-method adaptive")
    ap.add_argument("--adaptive-weight", type=float, default=1.0, metavar="POWER", help="the octree sampling splits the node with the largest count ** POWER first (0: all alike)")
    ap.add_argument("-a", "--append-ply", action="append", default=[],
                    help="a PLY file to append after the downsampling, relative to the input's folder unless absolute; may be repeated")
    ap.add_argument("-k", "--keep-strategy", choices=("centroid", "center", "first", "random"), default="centroid",
                    help="the point kept per voxel: nearest the centroid (default), nearest the voxel centre, the first, or a random one")
    ap.add_argument("--sky-axis", choices=SKY_AXIS_CHOICES, default=None, help="add a sky dome of points around this axis (needs --out)")
    ap.add_argument("--sky-scale", type=float, default=100.0, help="radius of the sky dome in the cloud's units")
    ap.add_argument("--sky-count", type=int, default=4000, help="points of the sky dome")
    ap.add_argument("--sky-percent", type=float, default=50.0, help="part of the sphere the dome covers: 50 = hemisphere, 100 = sphere")
    ap.add_argument("--sky-color", type=str, default="#87cefa", help="sky colour as #RRGGBB or R,G,B (0-255)")
    return ap


def is_colmap_text_model_dir(path):
    return path.is_dir() and all((path / name).is_file() for name in ("cameras.txt", "images.txt", "points3D.txt"))


def fail(text):
    print(f"[ERR] {text}")
    return 1


def main(argv=None):
    ap = create_arg_parser()
    args = ap.parse_args(argv)
    from gs360 import pointcloud

    if args.target_points is not None and args.target_points <= 0:
        ap.error("--target-points must be greater than 0")
    sky_color = None
    if args.sky_axis:
        if args.sky_scale is None or args.sky_scale <= 0:
            ap.error("--sky-scale must be > 0 when --sky-axis is set")
        if args.sky_count is None or args.sky_count <= 0:
            ap.error("--sky-count must be > 0 when --sky-axis is set")
        if args.sky_percent is None or not (0.0 < args.sky_percent <= 100.0):
            ap.error("--sky-percent must be > 0 and <= 100 when --sky-axis is set")
        try:
            sky_color = pointcloud._parse_sky_color(args.sky_color)
        except ValueError as exc:
            ap.error(f"--sky-color {exc}")

    adaptive = args.adaptive or args.downsample_method == "adaptive"
    try:
        refused = adaptive and args.output is not None and not pointcloud.adaptive_mode_from_env()
    except ValueError as exc:
        return fail(str(exc))
    if refused:
        return fail("--downsample-method adaptive is not built: the octree's split order is a serial priority queue")
    source_path = Path(os.path.expanduser(args.input)).resolve()
    if is_colmap_text_model_dir(source_path):
        return fail("a COLMAP text-model folder as input is not built: give a PLY file")

    import numpy as np
    from gs360 import capi
    xyz, rgb = pointcloud.load_ply_xyz_rgb(str(source_path))
    base_dir = str(source_path) if source_path.is_dir() else str(source_path.parent)
    print(f"[load] kind=ply base={source_path}  points={xyz.shape[0]:,}")
    stats = pointcloud.compute_point_cloud_stats(xyz)

    target_points = args.target_points if args.target_points and args.target_points > 0 else None
    if args.target_percent is not None:
        pct = args.target_percent
        if pct <= 0 or stats.count == 0:
            computed = 0
        else:
            computed = max(1, min(stats.count, int(round(stats.count * (pct / 100.0)))))
        print("[target-percent]", f"{pct:.6g}% of {stats.count:,} -> target_points={computed:,}")
        if computed > 0:
            if target_points is not None and target_points != computed:
                print("[target-percent] override", f"replacing explicit target_points={target_points:,}")
            target_points = computed
    has_target = target_points is not None and target_points > 0
    has_voxel = args.voxel_size is not None and args.voxel_size > 0
    pointcloud.print_point_cloud_stats(stats, include_voxel_reference=not has_target)

    if args.output is None:
        if has_voxel or has_target or args.adaptive or args.downsample_method != "voxel" or args.append_ply:
            print("[warn] --out missing; skipping downsample/append options.")
        else:
            print("[info] --out not provided; statistics only.")
        return 0

    how = args.keep_strategy
    try:
        if adaptive:
            if args.downsample_method != "adaptive":
                print("[warn] --adaptive is deprecated by --downsample-method; forcing method=adaptive.")
            adaptive_target = target_points if has_target else stats.count
            if adaptive_target == stats.count:
                print("[adaptive] target not specified; defaulting to input count (no reduction).")
            print("[adaptive] weight={:.3g} min_voxel={}".format(args.adaptive_weight, f"{args.voxel_size:.6g}" if has_voxel else "auto"))
            xyz, rgb = pointcloud.adaptive_voxel_downsample(xyz, rgb, adaptive_target, weight_power=args.adaptive_weight, stats=stats,
                                                            min_voxel_size=args.voxel_size if has_voxel else None, representative=how)
            print(f"[adaptive] target~{adaptive_target:,} -> {xyz.shape[0]:,} points")
        elif args.downsample_method == "spatial-hash":
            xyz, rgb = pointcloud.spatial_hash_downsample_one_pass(xyz, rgb, target_points=target_points,
                                                                   voxel_size=args.voxel_size if has_voxel else None, stats=stats,
                                                                   representative=how)
        elif has_voxel:
            print(f"[downsample] fixed voxel-size={args.voxel_size:.6g}")
            xyz, rgb = pointcloud.voxel_downsample_by_size(xyz, rgb, args.voxel_size, representative=how)
            print(f"[downsample] -> {xyz.shape[0]:,} points")
        elif has_target:
            xyz, rgb = pointcloud.voxel_downsample_to_target(xyz, rgb, target_points, stats=stats, log_bounds=False, representative=how)
            print(f"[downsample] target_points={target_points:,} -> {xyz.shape[0]:,} points")
        else:
            print("[downsample] skip (no voxel-size/target-points)")
    except capi.Gs360Error as exc:
        return fail(str(exc))
    finally:
        pointcloud.close_default_context()

    total_added = 0
    for apath in args.append_ply:
        full_path = os.path.expanduser(apath)
        if not os.path.isabs(full_path):
            full_path = os.path.join(base_dir, full_path)
        full_path = os.path.abspath(full_path)
        ax, ac = pointcloud.load_ply_xyz_rgb(full_path)
        xyz = np.concatenate([xyz, ax], axis=0)
        rgb = np.concatenate([rgb, ac], axis=0)
        total_added += ax.shape[0]
        print(f"[append] {full_path} +{ax.shape[0]:,} -> total {xyz.shape[0]:,}")
    if total_added > 0:
        print(f"[append] total added: {total_added:,}")

    if args.sky_axis:
        axis_vec = pointcloud._axis_direction(args.sky_axis)
        if axis_vec is None:
            ap.error(f"Invalid --sky-axis value: {args.sky_axis}")
        after = pointcloud.compute_point_cloud_stats(xyz)
        center = (after.xyz_min + after.xyz_max) * 0.5
        color = sky_color if sky_color is not None else np.array([135, 206, 250], dtype=np.uint8)
        sky_points, sky_colors = pointcloud._generate_sky_points(center.astype(np.float32, copy=False), axis_vec, float(args.sky_scale),
                                                                 int(args.sky_count), color, sky_percent=float(args.sky_percent))
        xyz = np.concatenate([xyz, sky_points], axis=0)
        rgb = np.concatenate([rgb, sky_colors], axis=0)
        print(f"[sky] axis={args.sky_axis} scale={args.sky_scale:.6g} percent={args.sky_percent:.6g} "
              f"count={sky_points.shape[0]:,} -> total {xyz.shape[0]:,}")

    out_path = Path(os.path.expanduser(args.output))
    if not out_path.is_absolute():
        out_path = out_path.resolve()
    pointcloud.save_ply_binary_little(str(out_path), xyz, rgb)
    print(f"[save] {out_path}  points={xyz.shape[0]:,}  (binary little-endian PLY)")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
