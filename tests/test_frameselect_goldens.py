"""The selection stage and the FrameSelector drop-in's whole main flow against the reference's own outputs on replayed scores
(tests/golden/frameselect_goldens.json, written by tests/golden/make_frameselect_goldens.py): stdout, CSV text and directory listing
character for character, and the eight selection functions' returned sets.  No GPU: main() takes the replayed scores and flow values
through its two seam keywords."""
import contextlib
import io
import json
import os
import pathlib
import re

import pytest

import gs360_FrameSelector as cli
from gs360 import frameselect as fsel

from conftest import GOLDEN

G = json.loads((GOLDEN / "frameselect_goldens.json").read_text())
IN_TOKEN, AUTO_TOKEN = G["tokens"]["in_dir"], G["tokens"]["auto_workers"]


def _listing(root):
    return sorted(str(p.relative_to(root)).replace(os.sep, "/") + ("/" if p.is_dir() else "") for p in pathlib.Path(root).rglob("*"))


def _tokenise(text, in_dir):
    """the two substitutions the goldens were written with: the input directory, and the machine's auto worker count"""
    text = text.replace(str(in_dir), IN_TOKEN)
    return re.sub(r"(\[INFO\] workers: .*auto=)\d+", lambda m: m.group(1) + AUTO_TOKEN, text)


def _populate(root, case):
    for k, name in enumerate(case["files"]):
        p = root / name
        p.write_bytes(b"name,score\nframe_0000.png,0.5\n" if name == "bad.csv" else b"")
        if case["mtimes"]:
            os.utime(p, (case["mtimes"][k], case["mtimes"][k]))


def test_the_goldens_cover_what_the_issue_lists():
    text = "\n".join(st["stdout"] + str(st["exit"]) for c in G["cases"].values() for st in c["steps"])
    for pattern in (r"Gap augmentation added [1-9]", r"Low-light augmentation added [1-9]", r"Motion augmentation added [1-9]",
                    r"Motion prune removed [1-9]", r"segment boundary reopt adjusted [1-9]", r"Optical flow computed for [1-9]",
                    r"Optical flow reused from reselect CSV", r" Skipped [1-9]", r"Pair mode requires complete", r"Input mode pair"):
        assert re.search(pattern, text), pattern
    assert all(60 <= sum(1 for f in c["files"] if not f.endswith((".txt", ".md", ".csv"))) <= 150
               for name, c in G["cases"].items() if not name.startswith("usage_no_images"))
    assert len(G["cases"]) >= 20 and all(len(v) >= 6 for v in G["functions"].values())


@pytest.mark.parametrize("name", sorted(G["cases"]))
def test_main_flow_equals_the_reference(name, tmp_path):
    case = G["cases"][name]
    scores = G["score_sets"][case["scores"]]
    flows = G["flow_sets"][case["flows"]] if case["flows"] else None
    _populate(tmp_path, case)
    for step in case["steps"]:
        for gone in step["remove"]:
            os.remove(tmp_path / gone)
        order = [case["files"][k] for k in step["order"]]
        by_name = {base: tuple(scores[k]) for k, base in enumerate(order)}

        def replay_scores(records, *a, **kw):
            assert [os.path.basename(r["primary_path"]) for r in records] == order
            return [by_name[os.path.basename(r["primary_path"])] for r in records]

        def replay_flow(records, flow_mag_arr, *a, **kw):
            for i in range(len(records)):
                flow_mag_arr[i] = max(flow_mag_arr[i], flows[i])
            return len(records) - 1
        cli.cancel_event.clear()
        out, code = io.StringIO(), None
        try:
            with contextlib.redirect_stdout(out):
                cli.main(["-i", str(tmp_path)] + step["argv"], score_records=replay_scores, flow_magnitudes=replay_flow)
        except SystemExit as e:
            code = e.code
        assert code == step["exit"]
        assert _tokenise(out.getvalue(), tmp_path) == step["stdout"]
        csvs = {p.name: p.read_text() for p in sorted(tmp_path.glob("*.csv")) if p.name != "bad.csv"}
        assert {k: G["csv_texts"][v] for k, v in step["csv"].items()} == csvs
        assert _listing(tmp_path) == step["listing"]


def _vectors(name):
    return [pytest.param(v, id=f"{name}-{k}") for k, v in enumerate(G["functions"][name])]


@pytest.mark.parametrize("v", _vectors("_spacing_respects"))
def test_spacing_respects(v):
    assert fsel._spacing_respects(*v["args"]) == v["out"]


@pytest.mark.parametrize("v", _vectors("_pick_even_candidate"))
def test_pick_even_candidate(v):
    existing, initial, sc, used, target, ordered, md, fw = v["args"]
    assert fsel._pick_even_candidate(existing, set(initial), sc, set(used), target, ordered, md, fw) == v["out"]


@pytest.mark.parametrize("v", _vectors("_pick_best_between"))
def test_pick_best_between(v):
    existing, sc, used, a, b, target, initial, ordered, md, fw = v["args"]
    assert fsel._pick_best_between(existing, sc, set(used), a, b, target, set(initial), ordered, md, fw) == v["out"]


@pytest.mark.parametrize("v", _vectors("augment_spacing"))
def test_augment_spacing(v):
    final, existing, sc, initial, ms, md, mode, fw = v["args"]
    assert sorted(fsel.augment_spacing(set(final), existing, sc, set(initial), ms, md, mode, fw)) == v["out"]


@pytest.mark.parametrize("v", _vectors("evenly_distribute_indices"))
def test_evenly_distribute_indices(v):
    existing, initial, sc, md, fw = v["args"]
    assert sorted(fsel.evenly_distribute_indices(existing, set(initial), sc, md, fw)) == v["out"]


@pytest.mark.parametrize("v", _vectors("augment_motion_segments"))
def test_augment_motion_segments(v):
    final, gi, existing, sc, flow, md = v["args"]
    assert sorted(fsel.augment_motion_segments(set(final), gi, existing, sc, flow, md)) == v["out"]


@pytest.mark.parametrize("v", _vectors("augment_lowlight_segments"))
def test_augment_lowlight_segments(v):
    final, gi, existing, sc, bm, md, kr, mk = v["args"]
    assert sorted(fsel.augment_lowlight_segments(set(final), gi, existing, sc, bm, md, kr, mk)) == v["out"]


@pytest.mark.parametrize("v", _vectors("refine_segment_selection_boundary_local"))
def test_refine_segment_selection_boundary_local(v, tmp_path):
    gi, sc, initial, md, tk, mp = v["args"]
    records = []
    for i in range(v["n"]):
        p = tmp_path / f"f{i:04d}.png"
        if i not in v["missing"]:
            p.write_bytes(b"")
        records.append({"file_paths": [str(p)]})
    assert sorted(fsel.refine_segment_selection_boundary_local(gi, records, sc, set(initial), md, tk, mp)) == v["out"]
