"""The (10, 8) instantiation's bounds and arithmetic, checked on the CPU: tests/tools/vidfeed_hostcheck.hip steps
vc_group<uint16_t, uint8_t> (csrc/gs360_vidsteps.h) on the host, built with AddressSanitizer and UndefinedBehaviorSanitizer and with
every plane and the destination at its exact size.  Every case must give the restatement's bytes (tests/vidfeed_np.py), leave the row
padding alone and draw no sanitizer report.  A stand-alone program: nothing is loaded into python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import vidcolor_np as ref
import vidfeed_np as feed_ref
from gs360 import vidcolor

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FILL = 0xA5
WIDTHS, HEIGHTS = (1, 7, 8, 9, 17, 24), (1, 2, 3, 5)
LAYOUTS = ("tight", "dword", "padded", "odd_dst", "off2")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc to build the host check with")
    if os.environ.get("LD_PRELOAD"):
        pytest.skip("a preloaded library and a sanitized program do not go together")
    exe = tmp_path_factory.mktemp("hostcheck") / "vidfeed_hostcheck"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "tools" / "vidfeed_hostcheck.hip")],
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


def strides_of(W, cw, layout):
    """-> (y, cb, cr, dst strides in bytes, luma pointer offset, whether the job is `fast`)"""
    rows = [2 * W, 2 * cw, 2 * cw, 3 * W]
    dword = [(r + 3) // 4 * 4 for r in rows]
    if layout == "tight":
        return rows, 0, all(r % 4 == 0 for r in rows)
    if layout == "dword":
        return dword, 0, True
    if layout == "padded":
        return [r + 8 for r in dword], 0, True
    if layout == "odd_dst":
        return dword[:3] + [dword[3] + 1], 0, False
    return dword, 2, False                                  # off2: the luma plane two bytes off its dword


def all_cases():
    for W in WIDTHS:
        for H in HEIGHTS:
            for sub in ("420", "422", "444"):
                for layout in LAYOUTS:
                    yield W, H, sub, layout, (W + H) % 2 == 1, (W // 2 + H) % 2 == 1     # both ranges and both curves across the cases


def test_every_group_of_every_case(program, tmp_path):
    rng = np.random.default_rng(1920)
    m, lin = vidcolor.primaries_matrix().astype(np.float32), vidcolor.linear_table()
    cases = list(all_cases())
    blob = [np.array([len(cases)], np.int32).tobytes(), m.tobytes(), lin.tobytes(), vidcolor.encode_table(False, 255).tobytes(),
            vidcolor.encode_table(True, 255).tobytes()]
    want = []
    n_fast = 0
    for W, H, sub, layout, full, keep in cases:
        ch, cw = ref.chroma_shape(H, W, sub)
        planes = [rng.integers(0, 1100, size=s).astype("<u2") for s in ((H, W), (ch, cw), (ch, cw))]     # samples above 1023 included
        planes[0].flat[0] = 65535
        strides, off, fast = strides_of(W, cw, layout)
        n_fast += fast
        sx, sy = ref.SUBS[sub]
        blob.append(np.array([W, H, sx, sy] + strides + [off, int(keep), 0, 0], np.int32).tobytes())
        blob.append(np.array(ref.coefficients(10, full), np.int32).tobytes())
        blob += [exact(p, s).tobytes() for p, s in zip(planes, strides[:3])]
        want.append((fast, strides[3], feed_ref.convert(*planes, sub, full, keep)))
    assert 0 < n_fast < len(cases) and any(np.any(p > 1023) for p in planes)
    (tmp_path / "in.bin").write_bytes(b"".join(blob))
    r = subprocess.run([str(program), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    got = np.fromfile(tmp_path / "out.bin", np.uint8)
    at = 0
    for (W, H, sub, layout, full, keep), (fast, ds, rgb) in zip(cases, want):
        what = (W, H, sub, layout, full, keep)
        tail = np.frombuffer(got[at:at + 8].tobytes(), np.int32)
        assert tail.tolist() == [int(fast), -(-W // 8) * -(-H // 2)], what
        n = (H - 1) * ds + 3 * W
        dst = got[at + 8:at + 8 + n]
        at += 8 + n
        inside = np.zeros(n, bool)
        for y in range(H):
            inside[y * ds:y * ds + 3 * W] = True
        assert dst.size == n and np.array_equal(dst[inside], exact(rgb.reshape(H, 3 * W), ds)[inside]), what
        assert np.all(dst[~inside] == FILL), (what, "row padding was written")
    assert at == got.size
