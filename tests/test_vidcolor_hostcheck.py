"""VID-COLOR v1's bounds and arithmetic, checked on the CPU: tests/tools/vidcolor_hostcheck.hip steps the kernel's own per-lane
functions (csrc/gs360_vidsteps.h) on the host, built with AddressSanitizer and UndefinedBehaviorSanitizer and with every plane and
the destination at its exact size.  Every fixture must give the restatement's bytes, leave the row padding alone and draw no
sanitizer report.  A stand-alone program: nothing is loaded into python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import vidcolor_np as ref
from gs360 import vidcolor

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FILL = 0xA5


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc to build the host check with")
    if os.environ.get("LD_PRELOAD"):
        pytest.skip("a preloaded library and a sanitized program do not go together")
    exe = tmp_path_factory.mktemp("hostcheck") / "vidcolor_hostcheck"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "tools" / "vidcolor_hostcheck.hip")],
                   check=True, capture_output=True, timeout=600)
    return exe


def exact(plane, stride):
    """rows `stride` bytes apart, the buffer ending with the last row"""
    H, row = plane.shape[0], plane.shape[1] * plane.itemsize
    buf = np.full((H - 1) * stride + row, 0x5A, np.uint8)
    raw = np.ascontiguousarray(plane).view(np.uint8).reshape(H, row)
    for y in range(H):
        buf[y * stride:y * stride + row] = raw[y]
    return buf


def check(program, tmp_path, W, H, sub, depth, pad, want_fast, full=False, keep=False):
    """pad: bytes added to every tight stride (0 = tight); ("dword", n) rounds the row up to a dword first"""
    rng = np.random.default_rng(W * 1000 + H * 10 + depth + len(sub))
    dt = np.uint8 if depth == 8 else np.dtype("<u2")
    ch, cw = ref.chroma_shape(H, W, sub)
    planes = [rng.integers(0, 1100 if depth == 10 else 256, size=s).astype(dt) for s in ((H, W), (ch, cw), (ch, cw))]
    item = np.dtype(dt).itemsize
    rows = [W * item, cw * item, cw * item, 3 * W * item]
    strides = [((r + 3) // 4 * 4 + pad[1]) if isinstance(pad, tuple) else r + pad for r in rows]
    sx, sy = ref.SUBS[sub]
    m, lin, enc = vidcolor.primaries_matrix().astype(np.float32), vidcolor.linear_table(), vidcolor.encode_table(keep, 255 if depth == 8 else 65535)
    head = np.array([depth, W, H, sx, sy] + strides + [0, 0, 0], np.int32).tobytes() + np.array(ref.coefficients(depth, full), np.int32).tobytes()
    (tmp_path / "in.bin").write_bytes(head + m.tobytes() + lin.tobytes() + enc.tobytes() + b"".join(exact(p, s).tobytes() for p, s in zip(planes, strides[:3])))
    r = subprocess.run([str(program), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    what = (W, H, sub, depth, pad)
    assert r.returncode == 0 and not r.stderr, (what, r.stderr[-3000:])
    fast, groups = (int(v) for v in r.stdout.split())
    assert (fast, groups) == (int(want_fast), -(-W // 8) * -(-H // 2)), what
    got = np.fromfile(tmp_path / "out.bin", np.uint8)
    want = exact(ref.convert(*planes, depth, sub, full, keep).reshape(H, 3 * W), strides[3])
    inside = np.zeros(got.size, bool)
    for y in range(H):
        inside[y * strides[3]:y * strides[3] + rows[3]] = True
    assert got.size == want.size and np.array_equal(got[inside], want[inside]), what
    assert np.all(got[~inside] == FILL), (what, "row padding was written")


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("sub", ["420", "422", "444"])
def test_odd_and_even_frames(program, tmp_path, sub, depth):
    """33 x 5 and 70 x 6, tight (dword rows only where the widths allow) and with every row rounded up to a dword (the group path
    with its pixel tail at both widths)"""
    for W, H in ((33, 5), (70, 6)):
        item = 1 if depth == 8 else 2
        rows = [W * item, ref.chroma_shape(H, W, sub)[1] * item, 3 * W * item]
        tight = all(r % 4 == 0 for r in rows)
        check(program, tmp_path, W, H, sub, depth, 0, tight)
        check(program, tmp_path, W, H, sub, depth, ("dword", 0), True)


def test_a_single_pixel(program, tmp_path):
    for depth in (8, 10):
        for sub in ("420", "422", "444"):
            check(program, tmp_path, 1, 1, sub, depth, 0, False)


def test_padded_and_odd_strides(program, tmp_path):
    for sub in ("420", "422", "444"):
        for depth in (8, 10):
            check(program, tmp_path, 9, 2, sub, depth, ("dword", 8), True)
        check(program, tmp_path, 9, 2, sub, 8, 3, False)         # odd byte strides: 12, 8 or 12, 30
        check(program, tmp_path, 9, 2, sub, 8, ("dword", 1), False)


def test_both_ranges_and_encodes(program, tmp_path):
    for full in (False, True):
        for keep in (False, True):
            check(program, tmp_path, 70, 6, "420", 10, ("dword", 0), True, full, keep)
            check(program, tmp_path, 33, 5, "420", 8, ("dword", 4), True, full, keep)
