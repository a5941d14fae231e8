"""The FrameSelector's selection stage: which frames of a scored sequence stay (cli_tools/gs360_FrameSelector.py, FS:1054-1915 and
the selection part of its main flow, FS:2426-2683).  Pure host logic on plain lists: `scores` holds a float or None per record,
`existing_indices` the sorted indices of the records whose files are on disk, a "group" is one segment {"start", "end", ...} of
consecutive record indices.  The functions a workflow patch would import keep the reference's names and signatures; behaviour is
pinned by tests/golden/frameselect_goldens.json (the reference's own outputs on replayed scores).

NumPy is used for np.percentile alone (the motion thresholds), so that the interpolation is the reference's.
"""
import bisect
import csv
import math
import os
import re
import shutil

import numpy as np

MOTION_ANISO_WEIGHT = 0.5              # FS:311-345
FLOW_DOWNSCALE = 320
FLOW_MOTION_WEIGHT = 0.6
FLOW_HIGH_MOTION_THRESHOLD = 0.5
FLOW_HIGH_MOTION_RATIO = 0.4
FLOW_LOW_MOTION_PERCENTILE = 10.0
FLOW_MISSING_HIGH_VALUE = 9999.0
FLOW_CROP_RATIO = 0.6
FAST_SPACING_WINDOW = 64
FAST_SPACING_MULTIPLIER = 4.0
SEGMENT_BOUNDARY_REOPT_TOP_K = 3
SEGMENT_BOUNDARY_REOPT_MAX_PASSES = 3
GROUP_BRIGHTNESS_POWER = 1.5
DEFAULT_CROP_RATIO = 0.8
MAX_LONG = 0
MAX_SPACING_FRAMES = 0
MAX_SPACING_RATIO = 0.8
BRIGHTNESS_SHARPNESS_KEEP_RATIO = 0.2
BRIGHTNESS_SHARPNESS_MIN_KEEP = 0
MIN_DIFF_FRAMES_RATIO = 0.2
DEFAULT_SCORE_BACKEND = "ffmpeg"
PAIR_X_SUFFIX = "_X"
PAIR_Y_SUFFIX = "_Y"

EXTS = {"tif": {".tif", ".tiff"}, "jpg": {".jpg", ".jpeg"}, "png": {".png"}}
ALL_EXTS = set().union(*EXTS.values())
CSV_HEADER = ["index", "input_mode", "filename", "pair_base", "x_filename", "y_filename", "score", "brightness_mean", "group_score",
              "flow_motion", "selected(1=keep)"]
CSV_ENCODINGS = ("utf-8-sig", "utf-8", "cp932")


def round_half_up(value):
    return int(math.floor(value + 0.5))


# ---- files, records, order -------------------------------------------------------------------------------------------------------
# The reference's number pattern is a raw string with a doubled backslash: it matches a literal backslash followed by "d"s, not
# digits, so an ordinary file name has no number group and "lastnum" / "firstnum" order by the lower-cased name.  The order fixes
# every record's index in the CSVs the GUI exchanges with the tool, so it is kept as it runs, not as its help text reads.
_NUMBER_GROUPS = re.compile(r"(\\d+)")


def _numbered_key(which):
    def key(path):
        base = os.path.basename(path)
        groups = _NUMBER_GROUPS.findall(os.path.splitext(base)[0])
        return (0, int(groups[which]), base.lower()) if groups else (1, base.lower())
    return key


def sort_key_name(path):
    return os.path.basename(path).lower()


def sort_key_mtime(path):
    try:
        return os.path.getmtime(path)
    except Exception:
        return 0.0


sort_key_lastnum = _numbered_key(-1)
sort_key_firstnum = _numbered_key(0)
SORTERS = {"lastnum": sort_key_lastnum, "firstnum": sort_key_firstnum, "name": sort_key_name, "mtime": sort_key_mtime}


def gather_files(in_dir, ext_mode="all"):
    """The image files directly in in_dir (no recursion) with a wanted extension, in listing order, each real path once."""
    wanted = ALL_EXTS if ext_mode == "all" else EXTS[ext_mode]
    seen, files = set(), []
    for name in os.listdir(in_dir):
        fp = os.path.join(in_dir, name)
        if not os.path.isfile(fp) or os.path.splitext(name)[1].lower() not in wanted:
            continue
        ident = os.path.normcase(os.path.abspath(fp))
        if ident not in seen:
            seen.add(ident)
            files.append(fp)
    return files


def split_stem_suffix(stem, x_suffix=PAIR_X_SUFFIX, y_suffix=PAIR_Y_SUFFIX):
    """(pair base, "X" / "Y" / "") of a file stem."""
    for suffix, lens in ((x_suffix, "X"), (y_suffix, "Y")):
        if stem.endswith(suffix):
            return stem[:-len(suffix)], lens
    return stem, ""


def _record(mode, name, base, paths, x_path="", y_path=""):
    return {"input_mode": mode, "display_name": name, "pair_base": base, "primary_path": paths[0], "file_paths": list(paths),
            "x_path": x_path, "y_path": y_path}


def build_pair_records(file_paths, sorter):
    """-> (pair records ordered by their X file, files without a lens suffix, bases that miss a lens)."""
    lenses, unmatched = {}, []
    for fp in file_paths:
        base, lens = split_stem_suffix(os.path.splitext(os.path.basename(fp))[0])
        if lens:
            lenses.setdefault(base, {})[lens] = fp
        else:
            unmatched.append(fp)
    pairs, incomplete = [], []
    for base, by_lens in lenses.items():
        x, y = by_lens.get("X"), by_lens.get("Y")
        if x and y:
            pairs.append(_record("pair", base, base, [x, y], x, y))
        else:
            incomplete.append(base)
    return sorted(pairs, key=lambda r: sorter(r["primary_path"])), unmatched, incomplete


def build_input_records(file_paths, input_mode, sorter):
    """-> (mode, records): one record per image, or per X / Y pair when the folder holds complete pairs only (mode "auto") or must
    (mode "pair": SystemExit otherwise)."""
    singles = sorted((_record("single", os.path.basename(fp), "", [fp]) for fp in file_paths), key=lambda r: sorter(r["primary_path"]))
    if input_mode == "single":
        return "single", singles
    pairs, unmatched, incomplete = build_pair_records(file_paths, sorter)
    clean = not unmatched and not incomplete
    if input_mode == "pair":
        if not clean:
            raise SystemExit("Pair mode requires complete _X/_Y image pairs only. "
                             "unmatched_files={}, incomplete_pairs={}".format(len(unmatched), len(incomplete)))
        if not pairs:
            raise SystemExit("Pair mode found no valid _X/_Y image pairs.")
        return "pair", pairs
    return ("pair", pairs) if pairs and clean else ("single", singles)


def record_exists(record):
    paths = record.get("file_paths", [])
    return bool(paths) and all(os.path.isfile(p) for p in paths)


def record_csv_labels(record):
    """(filename, pair_base, x_filename, y_filename) columns of a record's CSV row."""
    return (str(record.get("display_name", "") or os.path.basename(record["primary_path"])), str(record.get("pair_base", "") or ""),
            os.path.basename(record["x_path"]) if record.get("x_path") else "",
            os.path.basename(record["y_path"]) if record.get("y_path") else "")


def unique_path(dst_path):
    """dst_path, or the first of dst_1.ext, dst_2.ext, ... that does not exist."""
    if not os.path.exists(dst_path):
        return dst_path
    base, ext = os.path.splitext(dst_path)
    k = 1
    while os.path.exists("{}_{}{}".format(base, k, ext)):
        k += 1
    return "{}_{}{}".format(base, k, ext)


def safe_move(src, dst):
    """Move src to dst (never over an existing file); copy and delete when the move fails.  The final path, or None."""
    if not os.path.isfile(src):
        return None
    final = unique_path(dst)
    os.makedirs(os.path.dirname(final), exist_ok=True)
    try:
        shutil.move(src, final)
        return final
    except Exception:
        pass
    try:
        shutil.copy2(src, final)
    except Exception:
        return None
    try:
        os.remove(src)
    except Exception:
        pass
    return final


# ---- CSV in ----------------------------------------------------------------------------------------------------------------------
def _with_encodings(csv_path, read, reset=None):
    """read(DictReader) under the first of CSV_ENCODINGS that decodes the file; reset() before every retry."""
    error = None
    for encoding in CSV_ENCODINGS:
        try:
            with open(csv_path, "r", newline="", encoding=encoding) as f:
                return read(csv.DictReader(f))
        except UnicodeDecodeError as exc:
            error = exc
            if reset:
                reset()
    raise error


def load_selection_from_csv(csv_path, files, scores, brightness_mean_arr, group_score_arr, flow_mag_arr):
    """The keep flag per record from a CSV the tool wrote, and its score / brightness_mean / group_score / flow_motion columns into
    the given lists (a negative score is a failed record: None).  Rows address records by their index column."""
    n = len(files)
    flags = [0] * n
    columns = (("brightness_mean", brightness_mean_arr), ("group_score", group_score_arr), ("flow_motion", flow_mag_arr))

    def read(reader):
        if reader.fieldnames is None:
            raise ValueError("CSV file has no header")
        names = {name.lower(): name for name in reader.fieldnames}
        keep_key = names.get("selected(1=keep)", names.get("selected"))
        if keep_key is None:
            raise ValueError("CSV missing 'selected(1=keep)' column")
        index_key, score_key = names.get("index"), names.get("score")
        for row in reader:
            if index_key is None:
                raise ValueError("CSV missing 'index' column")
            try:
                idx = int(row[index_key])
            except (TypeError, ValueError):
                continue
            if not 0 <= idx < n:
                continue
            flags[idx] = 1 if str(row.get(keep_key, "0")).strip() in {"1", "true", "True"} else 0
            if score_key and row.get(score_key) not in (None, ""):
                try:
                    value = float(row[score_key])
                    scores[idx] = None if value < 0.0 else value
                except ValueError:
                    scores[idx] = None
            for name, arr in columns:
                key = names.get(name)
                if key and row.get(key) not in (None, ""):
                    try:
                        arr[idx] = float(row[key])
                    except ValueError:
                        pass
        return flags

    def reset():
        flags[:] = [0] * n
        scores[:] = [None] * n
        for _, arr in columns:
            arr[:] = [0.0] * n
    return _with_encodings(csv_path, read, reset)


def csv_has_numeric_flow_motion_values(csv_path):
    """Does the CSV hold at least one number in its flow_motion column."""
    def read(reader):
        if reader.fieldnames is None:
            return False
        key = {name.lower(): name for name in reader.fieldnames}.get("flow_motion")
        if key is None:
            return False
        for row in reader:
            text = "" if row.get(key) is None else str(row.get(key)).strip()
            try:
                float(text)
            except ValueError:
                continue
            return True
        return False
    return _with_encodings(csv_path, read)


# ---- spacing ---------------------------------------------------------------------------------------------------------------------
def _score_or_negative_infinity(scores, index):
    value = scores[index]
    return float("-inf") if value is None else float(value)


def _spacing_respects(sorted_selected, candidate, min_diff):
    """Is candidate at least min_diff away from both of its neighbours in sorted_selected."""
    if min_diff <= 1 or not sorted_selected:
        return True
    pos = bisect.bisect_left(sorted_selected, candidate)
    below = pos > 0 and candidate - sorted_selected[pos - 1] < min_diff
    above = pos < len(sorted_selected) and sorted_selected[pos] - candidate < min_diff
    return not below and not above


def _best_in_ranges(ranges, existing_indices, scores, used, target_pos, initial_selected, sorted_selected, min_diff):
    """The unused, scored, well-spaced frame with the largest (was an initial pick, score, nearness to target_pos, low index) among
    the positions of the first range that has one; a position counts once."""
    seen = set()
    for positions in ranges:
        best, best_key = None, None
        for pos in positions:
            if pos in seen:
                continue
            seen.add(pos)
            idx = existing_indices[pos]
            if idx in used or scores[idx] is None:
                continue
            if min_diff > 1 and not _spacing_respects(sorted_selected, idx, min_diff):
                continue
            key = (1 if idx in initial_selected else 0, float(scores[idx]), -abs(pos - target_pos), -idx)
            if best_key is None or key > best_key:
                best, best_key = idx, key
        if best is not None:
            return best
    return None


def _window_then_all(lo, hi, target_pos, fast_window):
    """Positions [lo, hi) near target_pos first, then all of [lo, hi) when the window left some out."""
    start, stop = max(lo, target_pos - fast_window), min(hi, target_pos + fast_window + 1)
    ranges = [range(start, stop)]
    if start > lo or stop < hi:
        ranges.append(range(lo, hi))
    return ranges


def _pick_even_candidate(existing_indices, initial_selected, scores, used, target_pos, sorted_selected, min_diff,
                         fast_window=FAST_SPACING_WINDOW):
    """The best frame near position target_pos of existing_indices (see _best_in_ranges), or None."""
    if not existing_indices:
        return None
    return _best_in_ranges(_window_then_all(0, len(existing_indices), target_pos, fast_window), existing_indices, scores, used,
                           target_pos, initial_selected, sorted_selected, min_diff)


def _pick_best_between(existing_indices, scores, used, start_pos, end_pos, target_pos, initial_selected, sorted_selected, min_diff,
                       fast_window=FAST_SPACING_WINDOW):
    """The best frame strictly between positions start_pos and end_pos, or None."""
    if end_pos - start_pos <= 1:
        return None
    return _best_in_ranges(_window_then_all(start_pos + 1, end_pos, target_pos, fast_window), existing_indices, scores, used,
                           target_pos, initial_selected, sorted_selected, min_diff)


def augment_spacing(final_selected, existing_indices, scores, initial_selected, max_spacing, min_diff, mode="single",
                    fast_window=FAST_SPACING_WINDOW):
    """Insert a frame in the middle of every gap wider than max_spacing positions.  Mode "single": one sweep over as many
    neighbour pairs as the selection had when the sweep began (it sees the gaps its own insertions open, and stops that many pairs
    short of the end).  Mode "strict": the sweep restarts after each insertion until one passes without any."""
    if max_spacing is None or max_spacing <= 0:
        return set(final_selected)
    strict = str(mode or "single").strip().lower() == "strict"
    position = {idx: pos for pos, idx in enumerate(existing_indices)}
    chosen = set(final_selected)
    ordered = sorted(chosen)
    while True:
        inserted = False
        for i in range(len(ordered) - 1):
            left, right = position.get(ordered[i]), position.get(ordered[i + 1])
            if left is None or right is None or right - left <= max_spacing:
                continue
            pick = _pick_best_between(existing_indices, scores, chosen, left, right, int(round((left + right) / 2.0)), initial_selected,
                                      ordered, min_diff, fast_window)
            if pick is None:
                continue
            chosen.add(pick)
            bisect.insort(ordered, pick)
            inserted = True
            if strict:
                break
        if not strict or not inserted:
            return chosen


def evenly_distribute_indices(existing_indices, initial_selected, scores, min_diff, fast_window):
    """As many frames as initial_selected holds, spread evenly over existing_indices while preferring initial picks and sharp
    frames; what the even targets cannot place is filled from the best of the rest."""
    want = len(initial_selected)
    if want <= 0:
        return set()
    if want >= len(existing_indices):
        return set(existing_indices)
    used, ordered = set(), []
    last = len(existing_indices) - 1
    step = last / max(want - 1, 1)
    for k in range(want):
        target = last // 2 if want == 1 else int(round(k * step))
        pick = _pick_even_candidate(existing_indices, initial_selected, scores, used, target, ordered, min_diff, fast_window)
        if pick is None:
            break
        used.add(pick)
        bisect.insort(ordered, pick)
    if len(ordered) < want:
        rest = sorted((idx for idx in existing_indices if idx not in used), reverse=True,
                      key=lambda idx: (1 if idx in initial_selected else 0, _score_or_negative_infinity(scores, idx), -idx))
        for idx in rest:
            if len(ordered) >= want:
                break
            if min_diff > 1 and not _spacing_respects(ordered, idx, min_diff):
                continue
            used.add(idx)
            bisect.insort(ordered, idx)
    return set(ordered)


# ---- per-segment augmentations ---------------------------------------------------------------------------------------------------
def augment_motion_segments(final_selected, group_infos, existing_indices, scores, flow_mag_arr, min_diff):
    """More frames in the segments that move: where a segment's largest flow reaches max(FLOW_HIGH_MOTION_THRESHOLD, P80 of the
    positive flows), add its highest-flow frames, min_diff apart from every chosen frame, up to what the spacing leaves room for
    and FLOW_HIGH_MOTION_RATIO of the segment."""
    moving = [v for v in flow_mag_arr if v > 0.0 and np.isfinite(v)]
    if not moving:
        return set(final_selected)
    threshold = max(FLOW_HIGH_MOTION_THRESHOLD, float(np.percentile(moving, 80.0)))
    chosen = set(final_selected)
    existing = set(existing_indices)
    ratio = max(0.0, min(1.0, FLOW_HIGH_MOTION_RATIO))
    for info in group_infos:
        start, end = info["start"], info["end"]
        members = [i for i in range(start, end) if i in existing and scores[i] is not None and np.isfinite(flow_mag_arr[i])]
        if not members:
            continue
        peak = max(flow_mag_arr[i] for i in members)
        if not np.isfinite(peak) or peak < threshold:
            continue
        span = max(1, end - start)
        budget = max(0, math.ceil(span / max(1, min_diff)) - sum(1 for i in chosen if start <= i < end))
        if budget and ratio > 0.0:
            budget = min(budget, max(1, round_half_up(span * ratio)))
        if budget <= 0:
            continue
        ranked = sorted((i for i in members if i not in chosen), reverse=True,
                        key=lambda i: (flow_mag_arr[i], _score_or_negative_infinity(scores, i), -i))
        for idx in ranked:
            if budget <= 0:
                break
            if min_diff > 1 and any(abs(idx - sel) < min_diff for sel in chosen):
                continue
            chosen.add(idx)
            budget -= 1
    return chosen


def augment_lowlight_segments(final_selected, group_infos, existing_indices, scores, brightness_mean_arr, min_diff, keep_ratio, min_keep):
    """More frames per segment by score * brightness_mean ^ GROUP_BRIGHTNESS_POWER: up to max(min_keep, round(span * keep_ratio))
    unselected scored frames of each segment, min_diff apart from their chosen neighbours."""
    if keep_ratio <= 0.0 and min_keep <= 0:
        return set(final_selected)
    chosen = set(final_selected)
    existing = set(existing_indices)

    def weighted(i):
        return float(scores[i]) * max(1e-6, float(brightness_mean_arr[i])) ** GROUP_BRIGHTNESS_POWER
    for info in group_infos:
        start, end = info["start"], info["end"]
        budget = max(int(round(max(1, end - start) * max(0.0, min(1.0, keep_ratio)))), int(min_keep))
        if budget <= 0:
            continue
        ranked = sorted((i for i in range(start, end) if i in existing and scores[i] is not None and i not in chosen), reverse=True,
                        key=lambda i: (weighted(i), _score_or_negative_infinity(scores, i), -i))
        ordered = sorted(chosen)
        for idx in ranked:
            if budget <= 0:
                break
            if min_diff > 1 and not _spacing_respects(ordered, idx, min_diff):
                continue
            chosen.add(idx)
            bisect.insort(ordered, idx)
            budget -= 1
    return chosen


# ---- boundary re-optimisation ----------------------------------------------------------------------------------------------------
def _group_center_index(info):
    start = int(info.get("start", 0))
    end = int(info.get("end", start + 1))
    return float(start) if end <= start else (float(start) + float(end - 1)) * 0.5


def _boundary_edge_penalty(left_idx, right_idx, left_info, right_info, min_diff):
    """(1 when the two picks are closer than min_diff, how far short of the distance of their segments' centres they fall, 0..1)."""
    if left_idx is None or right_idx is None:
        return 0, 0.0
    dist = abs(int(right_idx) - int(left_idx))
    target = max(1.0, abs(_group_center_index(right_info) - _group_center_index(left_info)))
    return (1 if min_diff > 1 and dist < min_diff else 0), max(0.0, target - float(dist)) / target


def _boundary_pair_objective(left_idx, right_idx, left_group, right_group, prev_idx, prev_group, next_idx, next_group, scores, min_diff,
                             initial_selected, current_left, current_right):
    """Larger is better, compared in order: fewer spacing violations over the (up to) three edges the pair touches, less
    shortfall, more sharpness, more initial picks, fewer changes."""
    edges = [(left_idx, right_idx, left_group, right_group)]
    if prev_group is not None:
        edges.append((prev_idx, left_idx, prev_group, left_group))
    if next_group is not None:
        edges.append((right_idx, next_idx, right_group, next_group))
    hard, shortfall = 0, 0.0
    for a, b, ga, gb in edges:
        h, s = _boundary_edge_penalty(a, b, ga, gb, min_diff)
        hard += h
        shortfall += s
    sharp = _score_or_negative_infinity(scores, left_idx) + _score_or_negative_infinity(scores, right_idx)
    return (-hard, -shortfall, sharp, int(left_idx in initial_selected) + int(right_idx in initial_selected),
            -(int(left_idx != current_left) + int(right_idx != current_right)))


def refine_segment_selection_boundary_local(group_infos, records, scores, initial_selected, min_diff,
                                            top_k=SEGMENT_BOUNDARY_REOPT_TOP_K, max_passes=SEGMENT_BOUNDARY_REOPT_MAX_PASSES):
    """One pick per segment, re-chosen pair by pair of neighbouring segments among each segment's top_k sharpest frames (and its
    current pick) by _boundary_pair_objective, for at most max_passes sweeps."""
    if not group_infos:
        return set(initial_selected)
    top_k, max_passes = max(1, int(top_k)), max(1, int(max_passes))
    initial = set(initial_selected)
    options, picked = [], []
    for info in group_infos:
        start = int(info.get("start", 0))
        end = int(info.get("end", start))
        on_disk = [i for i in range(start, end) if record_exists(records[i])]
        ranked = sorted((i for i in on_disk if scores[i] is not None and math.isfinite(scores[i])), key=lambda i: (-float(scores[i]), i))
        current = next((i for i in range(start, end) if i in initial), None)
        if current is None:
            current = ranked[0] if ranked else (on_disk[0] if on_disk else None)
        cands = ranked[:top_k]
        if current is not None and current not in cands:
            cands.append(current)
        options.append(cands)
        picked.append(current)
    count = len(group_infos)
    for _ in range(max_passes if count >= 2 else 0):
        changed = False
        for g in range(count - 1):
            if not options[g] or not options[g + 1]:
                continue
            now = (picked[g], picked[g + 1])
            before = (picked[g - 1], group_infos[g - 1]) if g > 0 else (None, None)
            after = (picked[g + 2], group_infos[g + 2]) if g + 2 < count else (None, None)
            best, best_key = now, None
            for left in options[g]:
                for right in options[g + 1]:
                    key = _boundary_pair_objective(left, right, group_infos[g], group_infos[g + 1], before[0], before[1], after[0],
                                                   after[1], scores, min_diff, initial, now[0], now[1])
                    if best_key is None or key > best_key:
                        best, best_key = (left, right), key
            if best != now:
                picked[g], picked[g + 1] = best
                changed = True
        if not changed:
            break
    return {i for i in picked if i is not None}


# ---- the main flow's selection steps (FS:2099-2141, 2426-2634, 2800-2837) ----------------------------------------------------------
def spacing_plan(segment_size, min_spacing_frames, augment_motion, apply_csv):
    """The run's spacing numbers -> dict: base_spacing_frames, max_spacing, min_diff, motion_min_diff, fast_window."""
    base = max(0, round_half_up(segment_size * MIN_DIFF_FRAMES_RATIO) if min_spacing_frames is None else min_spacing_frames)
    max_spacing = MAX_SPACING_FRAMES
    if not apply_csv and max_spacing <= 0:
        max_spacing = round_half_up(segment_size * MAX_SPACING_RATIO)
    min_diff = 1 if apply_csv else base + 1
    motion_min_diff = max(0, base // 2) + 1 if augment_motion and not apply_csv else min_diff
    fast_window = max(1, round_half_up(segment_size * FAST_SPACING_MULTIPLIER)) if segment_size and segment_size > 0 else FAST_SPACING_WINDOW
    return {"base_spacing_frames": base, "max_spacing": max_spacing, "min_diff": min_diff, "motion_min_diff": motion_min_diff,
            "fast_window": fast_window}


def select_per_frame(scores, existing_indices, blur_percent):
    """Per-frame mode (segment size 0 or 1): all finitely scored frames on disk but the blur_percent lowest."""
    fraction = max(0.0, min(float(blur_percent), 100.0)) / 100.0
    ranked = sorted((i for i in existing_indices if scores[i] is not None and math.isfinite(scores[i])), key=lambda i: (scores[i], i))
    drop = round_half_up(len(ranked) * fraction) if fraction > 0.0 else 0
    return set(ranked[max(0, min(len(ranked), drop)):])


def group_segments(scores, brightness_arr, brightness_mean_arr, segment_size, group_score_arr):
    """Segments of segment_size consecutive records -> group infos; every member's group_score_arr entry becomes its segment's
    sum of score * brightness weight * brightness_mean ^ GROUP_BRIGHTNESS_POWER over the positively scored frames."""
    total = len(scores)
    infos = []
    for start in range(0, total, segment_size):
        end = min(total, start + segment_size)
        valid = [i for i in range(start, end) if scores[i] is not None]
        group_sum = 0.0
        for i in valid:
            if scores[i] > 0.0:
                group_sum += scores[i] * (brightness_arr[i] * (max(brightness_mean_arr[i], 1e-6) ** GROUP_BRIGHTNESS_POWER))
        group_score_arr[start:end] = [group_sum] * (end - start)
        infos.append({"start": start, "end": end, "valid_idx": valid, "group_sum": group_sum})
    return infos


def initial_picks(group_infos, scores, existing_indices):
    """The sharpest scored frame on disk of every segment (the first index among equals), else the segment's first frame on disk."""
    existing = set(existing_indices)
    picks = set()
    for info in group_infos:
        on_disk = [i for i in range(info["start"], info["end"]) if i in existing]
        scored = [i for i in on_disk if scores[i] is not None]
        if scored:
            picks.add(max(scored, key=lambda i: (scores[i], -i)))
        elif on_disk:
            picks.add(on_disk[0])
    return picks


def prune_low_motion(final_selected, flow_mag_arr):
    """The motion prune's choice -> (indices to drop, threshold): the threshold is P10 of the selected frames' flows; within every
    run of consecutive records at or below it (longer than two), the selected inner frame of least flow goes when its nearest
    selected neighbour in the run is as slow.  (set(), None) when no selected frame has a finite flow."""
    def finite(v):
        return v is not None and math.isfinite(v)
    values = [flow_mag_arr[i] for i in final_selected if finite(flow_mag_arr[i])]
    if not values:
        return set(), None
    threshold = float(np.percentile(values, FLOW_LOW_MOTION_PERCENTILE))

    def slow(i):
        return finite(flow_mag_arr[i]) and flow_mag_arr[i] <= threshold
    ordered = sorted(final_selected)
    dropped = set()
    n = len(flow_mag_arr)
    start = None
    for i in range(n + 1):
        if i < n and slow(i):
            start = i if start is None else start
            continue
        if start is None:
            continue
        first, last, start = start, i - 1, None
        if last - first < 2:
            continue
        inside = ordered[bisect.bisect_left(ordered, first):bisect.bisect_left(ordered, last + 1)]
        pool = [k for k in inside if first < k < last and slow(k)]
        if len(inside) < 2 or not pool:
            continue
        victim = min(pool, key=lambda k: (flow_mag_arr[k], k))
        nearest = min((k for k in inside if k != victim), key=lambda k: abs(k - victim), default=None)
        if nearest is not None and slow(nearest):
            dropped.add(victim)
    return dropped, threshold


def flow_summary(flow_mag_arr):
    """(min, median, max) of the finite flows below FLOW_MISSING_HIGH_VALUE, or None when there is none."""
    values = sorted(float(v) for v in flow_mag_arr if v is not None and math.isfinite(v) and float(v) < FLOW_MISSING_HIGH_VALUE)
    if not values:
        return None
    mid = len(values) // 2
    median = values[mid] if len(values) % 2 else (values[mid - 1] + values[mid]) * 0.5
    return values[0], median, values[-1]
