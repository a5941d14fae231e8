"""The inpaint stage's bounds and arithmetic, checked on the CPU: tests/tools/maskinpaint_hostcheck.hip steps the kernels' own per-lane
functions (csrc/gs360_maskinpaint.hip) on the host, built with AddressSanitizer and UndefinedBehaviorSanitizer and with every buffer
at its exact size.  Every fixture must give the restatement's bytes and K, a clear error word and no sanitizer report.  A
stand-alone program: nothing is loaded into python."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from gs360 import maskfinish

import maskinpaint_np as ref

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc to build the host check with")
    if os.environ.get("LD_PRELOAD"):
        pytest.skip("a preloaded library and a sanitized program do not go together")
    exe = tmp_path_factory.mktemp("hostcheck") / "maskinpaint_hostcheck"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "tools" / "maskinpaint_hostcheck.hip")],
                   check=True, capture_output=True, timeout=600)
    return exe


def run(program, tmp_path, img, F, radius=5, reverse=False):
    H, W = F.shape
    pairs, rlen, inv2 = maskfinish.inpaint_offsets(radius)
    (tmp_path / "in.bin").write_bytes(struct.pack("4i", H, W, radius, len(pairs)) + pairs.tobytes() + rlen.tobytes() + inv2.tobytes() +
                                      np.ascontiguousarray(img).tobytes() + np.where(F, 255, 0).astype(np.uint8).tobytes())
    r = subprocess.run([str(program), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")] + (["reverse"] if reverse else []),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    K, listed, err = (int(v) for v in r.stdout.split())
    return np.fromfile(tmp_path / "out.bin", np.uint8).reshape(H, W, 3), K, listed, err


def check(program, tmp_path, name, img, F, radius=5, reverse=False):
    want, K = ref.inpaint(img, F, radius)
    got, k, listed, err = run(program, tmp_path, img, F, radius, reverse)
    assert err == 0 and k == K, (name, k, K, err)
    assert listed == (int(F.sum()) if K else 0), name
    assert np.array_equal(got, want), (name, int((got != want).any(axis=2).sum()))


def test_the_specs_fixture_in_two_orders(program, tmp_path):
    F = ref.fixture_mask()
    H, W = F.shape
    for name, img in (("photo", ref.photograph(H, W, 5)), ("ramp", ref.ramp(H, W, 2, 3, 7))):
        check(program, tmp_path, name, img, F)
        check(program, tmp_path, name + "-reverse", img, F, reverse=True)


def test_sizes_past_a_tile_and_of_one(program, tmp_path):
    """a row longer than one workgroup's 256 pixels, sides of one, a single pixel outside F, every border touched"""
    rng = np.random.default_rng(3)
    wide = ref.discs(21, 300, [(10, 40), (8, 250), (20, 299)], 7)
    check(program, tmp_path, "21x300", ref.photograph(21, 300, 1), wide)
    check(program, tmp_path, "1x70", ref.photograph(1, 70, 2), rng.random((1, 70)) < 0.8)
    check(program, tmp_path, "70x1", ref.photograph(70, 1, 3), rng.random((70, 1)) < 0.8)
    lone = np.ones((9, 9), bool)
    lone[3, 5] = False
    check(program, tmp_path, "9x9-lone", ref.photograph(9, 9, 4), lone)
    frame = np.ones((30, 37), bool)
    frame[12:15, 17:21] = False
    check(program, tmp_path, "30x37-frame", ref.photograph(30, 37, 5), frame)


def test_one_region_with_levels_longer_than_a_workgroup(program, tmp_path):
    """the device test's limit fixture (tests/test_mask_limits_gpu.py): a disc of radius 60 over the row tile seam at x = 256"""
    check(program, tmp_path, "140x300-disc60", ref.photograph(140, 300, 5), ref.discs(140, 300, [(70, 230)], 60))


def test_the_other_radii_and_noise(program, tmp_path):
    F = ref.fixture_mask()
    noise = np.random.default_rng(9).choice(np.array([0, 255], np.uint8), size=F.shape + (3,))
    check(program, tmp_path, "noise", noise, F)
    for radius in (3, 8):
        check(program, tmp_path, f"radius-{radius}", ref.photograph(*F.shape, 6), F, radius)


def test_full_and_empty_masks_and_a_region_too_deep(program, tmp_path):
    img = ref.photograph(12, 9, 1)
    for F in (np.zeros((12, 9), bool), np.ones((12, 9), bool)):
        got, K, listed, err = run(program, tmp_path, img, F)
        assert (K, listed, err) == (0, 0, 0) and np.array_equal(got, img)
    deep = np.ones((1, 4200), bool)
    deep[0, 0] = False
    img = ref.photograph(1, 4200, 2)
    got, K, _listed, err = run(program, tmp_path, img, deep)
    assert K == 4096 and err == 0 and np.array_equal(got, img)       # the level the call refuses; nothing is filled
