"""The shadow estimate's bounds and arithmetic, checked on the CPU: tests/tools/maskshadow_hostcheck.hip steps the kernels' own
per-lane functions (csrc/gs360_maskshadow.hip, and csrc/gs360_maskmorph.hip for the morphology) on the host, built with
AddressSanitizer and UndefinedBehaviorSanitizer and with every buffer at its exact size.  Every fixture must give the restatement's
planes and counts, a clear error word and no sanitizer report.  A stand-alone program: nothing is loaded into python."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from gs360 import maskfinish

import maskshadow_cases as cases
import maskshadow_np as ref

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
STAGES = ("P", "C0", "C1", "C2", "clean")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc to build the host check with")
    if os.environ.get("LD_PRELOAD"):
        pytest.skip("a preloaded library and a sanitized program do not go together")
    exe = tmp_path_factory.mktemp("hostcheck") / "maskshadow_hostcheck"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "tools" / "maskshadow_hostcheck.hip")],
                   check=True, capture_output=True, timeout=600)
    return exe


def rows_bytes(rows):
    return np.asarray(rows, np.int32).tobytes()


def check(program, tmp_path, name, job):
    want = ref.run_job(job)
    H, W = job.raw.shape
    close = max(1, int(job.close))
    crows, ckw, ckh = (maskfinish.structuring_rows(close, close)[0], close, close) if close > 1 else ([], 0, 0)
    near, sclose, opening = ref.elements_of(job, want["count_p"])
    head = struct.pack("16i", H, W, job.thresh, ckw, ckh, len(job.half) - 1, job.sat_max, job.min_area, near[1], near[2], sclose[1], sclose[2],
                       opening[1], opening[2], 1, 0) + struct.pack("2f", job.t, job.delta_min)
    (tmp_path / "in.bin").write_bytes(head + b"".join(rows_bytes(r) for r in (crows, near[0], sclose[0], opening[0])) +
                                      np.asarray(job.half, np.float32).tobytes() + maskfinish.sat_div_table().tobytes() +
                                      job.raw.tobytes() + job.img.tobytes())
    r = subprocess.run([str(program), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (name, r.stderr[-3000:])
    count_p, count_m, err = (int(v) for v in r.stdout.split())
    got = np.fromfile(tmp_path / "out.bin", np.uint8).reshape(6, H, W)
    for k, stage in enumerate(STAGES):
        assert np.array_equal(got[k].astype(bool), want[stage]), (name, stage, int((got[k].astype(bool) != want[stage]).sum()))
    assert np.array_equal(got[5], np.where(want["M"], 255, 0)), (name, "M")
    assert (count_p, count_m, err) == (want["count_p"], want["count"], 0), name


def test_the_blur_and_candidate_fixtures(program, tmp_path):
    """every size of the device test: sides of 1, sides below the radius, both sides below 2 r + 1, past every tile"""
    for name, c in cases.blur_cases().items():
        check(program, tmp_path, name, cases.blur_job(c))


def test_the_label_fixtures(program, tmp_path):
    H, W = cases.LABEL_SIZES[0]
    for name, X in cases.label_planes(H, W).items():
        check(program, tmp_path, f"{H}x{W}-{name}", cases.label_job(name, X))


def test_two_label_fixtures_past_one_area_band_and_one_morph_tile(program, tmp_path):
    H, W = cases.LABEL_SIZES[1]
    planes = cases.label_planes(H, W)
    for name in ("spiral", "seams"):
        check(program, tmp_path, f"{H}x{W}-{name}", cases.label_job(name, planes[name]))


def test_the_fixtures_past_a_row_segment_at_the_largest_radius_and_past_two_tile_columns(program, tmp_path):
    """the device test's limit fixtures (tests/test_mask_limits_gpu.py): the row pass's second segment, r = 255 on a full segment
    (the last float of the staged row) and on a plane smaller than r both ways (the tallest staged column tile), each under the
    Gaussian and under the two outermost taps alone, and two labelling planes 2100 wide"""
    for name, job in cases.blur_limit_jobs().items():
        check(program, tmp_path, name, job)
    H, W = cases.LABEL_WIDE
    planes = cases.label_planes(H, W)
    for name in ("spiral", "seams"):
        check(program, tmp_path, f"{H}x{W}-{name}", cases.wide_label_job(name, planes[name]))


def test_the_photographs(program, tmp_path):
    check(program, tmp_path, "photo-97x130", cases.photo_job(97, 130, 12))
    check(program, tmp_path, "photo-97x130-nobody", cases.photo_job(97, 130, 12, person=False))
