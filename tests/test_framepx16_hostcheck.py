"""The FrameSelector passes' shared per-pixel steps on 16-bit samples, checked on the CPU: tests/tools/framepx16_hostcheck.hip calls
the host-callable steps of csrc/gs360_framepx.h on a buffer of its exact size, built with AddressSanitizer and
UndefinedBehaviorSanitizer.  Every pixel must give the model's values (tests/framescore16_np.py) and no sanitizer report, also when
the pixels start at an odd byte offset.  A stand-alone program: nothing is loaded into python."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import framescore16_np as fnp16
from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc to build the host check with")
    if os.environ.get("LD_PRELOAD"):
        pytest.skip("a preloaded library and a sanitized program do not go together")
    exe = tmp_path_factory.mktemp("hostcheck") / "framepx16_hostcheck"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "tools" / "framepx16_hostcheck.hip")],
                   check=True, capture_output=True, timeout=600)
    return exe


def _pixels(C):
    """Random pixels, the corners of the sample range, and grays on both sides of the highlight threshold."""
    rng = np.random.default_rng(16 + C)
    px = rng.integers(0, 65536, size=(4000, C), dtype=np.uint16)
    edge = np.array([0, 1, 255, 256, 257, 62193, 62194, 62258, 62259, 62260, 62450, 62451, 65534, 65535], np.uint16)
    same = np.repeat(edge[:, None], C, axis=1)                       # r = g = b = v: gray = v (the coefficients sum to 2^14)
    mixed = np.stack([np.roll(edge, k) for k in range(C)], axis=1)
    return np.concatenate([px, same, mixed])


@pytest.mark.parametrize("C,red,offset", [(1, 0, 0), (1, 0, 1), (3, 0, 0), (3, 2, 3), (4, 2, 5), (4, 0, 0)])
def test_steps_equal_the_model(program, tmp_path, C, red, offset):
    px = _pixels(C)
    n = px.shape[0]
    blob = struct.pack("<4i", C, red, offset, n) + bytes([0xA5] * offset) + px.tobytes()
    (tmp_path / "in.bin").write_bytes(blob)
    r = subprocess.run([str(program), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.fromfile(tmp_path / "out.bin", np.uint32).reshape(n, 5)
    img = px.reshape(1, n, C) if C > 1 else px.reshape(1, n)
    g16 = fnp16.gray_u16(img, red)[0]
    assert np.array_equal(got[:, 0], g16)
    if C > 1:
        rows = px[:, [red, 1, 2 - red]].astype(np.int64)
        assert np.array_equal(g16, (rows[:, 0] * 4899 + rows[:, 1] * 9617 + rows[:, 2] * 1868 + 8192) >> 14)
    from framescore_np import gray_u8
    assert np.array_equal(got[:, 1], gray_u8(fnp16.view8(img), red)[0])
    assert np.array_equal(got[:, 2], (g16 >= fnp16.HIGHLIGHT16).astype(np.uint32))
    assert np.array_equal(got[:, 3], (g16 + 192) // 257)
    assert np.array_equal(got[:, 3] >= 243, got[:, 2] == 1)           # plane 1's level carries the same highlight test
    assert np.array_equal(got[:, 4], (g16.astype(np.float32) * fnp16.SCALE32).view(np.uint32))
    assert 0 < got[:, 2].sum() < n
