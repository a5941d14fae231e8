"""The mask-finishing kernels' bounds and arithmetic, checked on the CPU: tests/tools/maskmorph_hostcheck.hip steps the kernels' own
per-lane functions (csrc/gs360_maskmorph.hip) on the host, built with AddressSanitizer and UndefinedBehaviorSanitizer and with every
buffer at its exact size.  Every fixture must give the restatement's pixels, count and checksum and no sanitizer report.  A stand-alone
program: nothing is loaded into python."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from gs360 import maskfinish

import maskfinish_cases as cases
import maskfinish_np as ref

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CASES = cases.cases()
LIMITS = cases.limit_cases()


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc to build the host check with")
    if os.environ.get("LD_PRELOAD"):
        pytest.skip("a preloaded library and a sanitized program do not go together")
    exe = tmp_path_factory.mktemp("hostcheck") / "maskmorph_hostcheck"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "tools" / "maskmorph_hostcheck.hip")],
                   check=True, capture_output=True, timeout=600)
    return exe


def fnv1a(data):
    h = 1469598103934665603
    for v in np.frombuffer(data, np.uint8).tolist():
        h = ((h ^ v) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def run(program, tmp_path, case, kind="mask", invert=True):
    """-> (count, checksum, the output array) of the host-stepped chain on one fixture"""
    H, W = cases.shape_of(case)
    jobs, _keep = maskfinish.build_jobs([(H, W)], case.params, kind, invert)
    j = jobs[0]
    rows = [np.asarray(maskfinish.structuring_rows(kw, kh)[0], np.int32).tobytes() if kh else b"" for kw, kh in
            ((j.close_kw, j.close_kh), (j.expand_kw, j.expand_kh))]
    head = struct.pack("16i", H, W, j.thresh, j.close_kw, j.close_kh, j.expand_kw, j.expand_kh, j.fuse, j.spread, j.kind, j.invert,
                       case.raw is not None, case.add is not None, 0, 0, 0)
    img = cases.image_for((H, W)) if kind != "mask" else None
    (tmp_path / "in.bin").write_bytes(head + rows[0] + rows[1] + (case.raw.tobytes() if case.raw is not None else b"") +
                                      (case.add.tobytes() if case.add is not None else b"") + (img.tobytes() if img is not None else b""))
    r = subprocess.run([str(program), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    count, digest = r.stdout.split()
    C = {"mask": 1, "rgba": 4, "keep": 3, "remove": 3}[kind]
    out = np.fromfile(tmp_path / "out.bin", np.uint8).reshape((H, W) if C == 1 else (H, W, C))
    return int(count), int(digest, 16), out, img


def check(program, tmp_path, name, kind="mask", invert=True):
    case = CASES[name] if name in CASES else LIMITS[name]
    count, digest, got, img = run(program, tmp_path, case, kind, invert)
    want, n = ref.finish(case.raw, case.params, case.add, img, kind, invert, cases.shape_of(case))
    assert np.array_equal(got, want), (name, kind)
    assert count == n and digest == fnv1a(want.tobytes()), (name, kind)


def test_every_small_fixture_equals_the_restatement_without_a_sanitizer_report(program, tmp_path):
    for name in CASES:
        if not name.startswith("big-"):
            check(program, tmp_path, name)


def test_the_fixture_past_one_tile_and_one_band(program, tmp_path):
    """515 x 1030 with a 155 x 155 element: 17 x 2 tiles, three bands of element rows, the wide-window path"""
    check(program, tmp_path, "big-crowd-p77")


def test_the_fixtures_past_the_tiles_at_the_largest_element_and_with_wide_strips(program, tmp_path):
    """the device test's limit fixtures (tests/test_mask_limits_gpu.py): a 1025 x 1025 element (halo 18: the whole 68-dword staged
    row, 16 bands) over two morph tile columns, three pack and output tile columns, side strips of seven dwords; one of them composed,
    where a lane has one pixel"""
    for name in LIMITS:
        check(program, tmp_path, name)
    check(program, tmp_path, "33x2100-corners", "rgba")


@pytest.mark.parametrize("kind", ["rgba", "keep", "remove"])
def test_the_compose_kinds_and_their_empty_branches(program, tmp_path, kind):
    some = next(n for n in CASES if n.startswith("40x33-disc"))
    for name in (some, "none-empty", "none-add-only"):
        for invert in (True, False):
            check(program, tmp_path, name, kind, invert)
