"""VID-FISHEYE v1's bounds and arithmetic, checked on the CPU: tests/tools/vidfisheye_hostcheck.hip steps the kernel's own per-lane
functions (csrc/gs360_vidfishsteps.h) on the host, built with AddressSanitizer and UndefinedBehaviorSanitizer and with every plane
and the destination at its exact size.  Every fixture must give the restatement's bytes, leave the row padding alone and draw no
sanitizer report.  A stand-alone program: nothing is loaded into python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import vidcolor_np as vc
import vidfisheye_np as ref
from gs360 import vidcolor

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FILL = 0xA5
VIEW = (120.0, 150.0, 150.0)          # lens circle 120 degrees, view 150: about half of the view looks past the lens
PROJ = {"equidistant": 0, "equisolid": 1}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc to build the host check with")
    if os.environ.get("LD_PRELOAD"):
        pytest.skip("a preloaded library and a sanitized program do not go together")
    exe = tmp_path_factory.mktemp("hostcheck") / "vidfisheye_hostcheck"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "tools" / "vidfisheye_hostcheck.hip")],
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


def stride_of(layout, row, item):
    if layout == "tight":
        return row
    padded = (row + 3) // 4 * 4 + 8
    if layout == "padded":
        return padded
    return ((row + 1) | 1) if item == 1 else padded + 2          # no multiple of 4; even for 16-bit samples


def check(program, tmp_path, W, H, S, sub, depth, layout, projection, full=False, keep=False):
    rng = np.random.default_rng(W * 1000 + H * 10 + depth + len(sub) + S)
    dt = np.uint8 if depth == 8 else np.dtype("<u2")
    ch, cw = vc.chroma_shape(H, W, sub)
    planes = [rng.integers(0, 1100 if depth == 10 else 256, size=s).astype(dt) for s in ((H, W), (ch, cw), (ch, cw))]
    item = np.dtype(dt).itemsize
    rows = [W * item, cw * item, cw * item, 3 * S * item]
    strides = [stride_of(layout, r, item) for r in rows]
    sx, sy = vc.SUBS[sub]
    c = ref.constants(projection, S, W, H, *VIEW)
    view = np.array([c[k] for k in ("tx", "ty", "kx32", "ky32", "kx16", "ky16", "ox32", "oy32", "ox16", "oy16")], np.float32)
    m, lin, enc = vidcolor.primaries_matrix().astype(np.float32), vidcolor.linear_table(), vidcolor.encode_table(keep, 255 if depth == 8 else 65535)
    head = np.array([depth, W, H, sx, sy] + strides + [S, PROJ[projection], 0], np.int32).tobytes() + np.array(vc.coefficients(depth, full), np.int32).tobytes()
    (tmp_path / "in.bin").write_bytes(head + view.tobytes() + m.tobytes() + lin.tobytes() + enc.tobytes() +
                                      b"".join(exact(p, s).tobytes() for p, s in zip(planes, strides[:3])))
    r = subprocess.run([str(program), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    what = (W, H, S, sub, depth, layout, projection)
    assert r.returncode == 0 and not r.stderr, (what, r.stderr[-3000:])
    fast, pixels = (int(v) for v in r.stdout.split())
    assert (fast, pixels) == (int(all(s % 4 == 0 for s in strides[:3])), S * S), what
    got = np.fromfile(tmp_path / "out.bin", np.uint8)
    want = exact(ref.render(*planes, depth, sub, projection, S, *VIEW, full, keep).reshape(S, 3 * S), strides[3])
    inside = np.zeros(got.size, bool)
    for y in range(S):
        inside[y * strides[3]:y * strides[3] + rows[3]] = True
    assert got.size == want.size and np.array_equal(got[inside], want[inside]), what
    assert np.all(got[~inside] == FILL), (what, "row padding was written")


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("sub", ["420", "422", "444"])
@pytest.mark.parametrize("layout", ["tight", "padded", "odd"])
def test_sources_and_views(program, tmp_path, layout, sub, depth):
    """sources 1 x 1, 2 x 2, 33 x 5 and 48 x 32 into views of 1, 7 and 64; the projection alternates"""
    k = 0
    for W, H in ((1, 1), (2, 2), (33, 5), (48, 32)):
        for S in (1, 7, 64):
            check(program, tmp_path, W, H, S, sub, depth, layout, ("equisolid", "equidistant")[k & 1])
            k += 1


def test_both_ranges_and_encodes(program, tmp_path):
    for full in (False, True):
        for keep in (False, True):
            check(program, tmp_path, 48, 32, 64, "420", 10, "padded", "equidistant", full, keep)
            check(program, tmp_path, 33, 5, 7, "420", 8, "padded", "equisolid", full, keep)
