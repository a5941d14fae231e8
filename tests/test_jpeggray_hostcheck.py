"""The gray output mode of the device JPEG decoder (gs360_jpeg_decode_gray_u8), checked on the CPU: tests/tools/jpeggray_hostcheck.hip
steps the kernels' own stage functions (csrc/gs360_jpegdec.hip) lane by lane on the host, the pixels step in gray mode, built with
AddressSanitizer and UndefinedBehaviorSanitizer and with the output plane at exactly H x stride bytes.  Every file must give FS-SPEC's
gray of Pillow's pixels, byte for byte, with status 0 and no sanitizer report: three bytes per pixel, or an x * C address into the
one-byte plane, ends the program.  A stand-alone program: nothing is loaded into python."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

pytest.importorskip("PIL.Image")

from conftest import ROOT  # noqa: E402
from gs360 import jpegdec  # noqa: E402

import jpegdec_cases as cases  # noqa: E402
import jpeggray_cases as gc  # noqa: E402

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc to build the host check with")
    if os.environ.get("LD_PRELOAD"):
        pytest.skip("a preloaded library and a sanitized program do not go together")
    exe = tmp_path_factory.mktemp("hostcheck") / "jpeggray_hostcheck"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "tools" / "jpeggray_hostcheck.hip")],
                   check=True, capture_output=True, timeout=600)
    return exe


def run(program, tmp_path, data, pad):
    """-> (status, the H x (W + pad) plane) of the host-stepped gray decode of one file"""
    d = jpegdec.parse(data, samplings=jpegdec.DEVICE_SAMPLINGS)
    seg, n_sub = jpegdec.segment_table(d)
    head = struct.pack("16i", d.H, d.W, d.C, d.subsampling, d.restart, d.scan_len, seg.shape[0], n_sub, 0, 0, 0, pad, 0, 0, 0, 0)
    sel = bytes((d.comp_tq + [0] * 4)[:4] + (d.comp_td + [0] * 4)[:4] + (d.comp_ta + [0] * 4)[:4])
    (tmp_path / "in.bin").write_bytes(head + sel + data[d.scan_off:d.scan_off + d.scan_len] + seg.tobytes() + d.huff.tobytes() + d.quant.tobytes())
    r = subprocess.run([str(program), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    words = r.stdout.split()
    assert words[words.index("sampling") + 1] == "%dx%d" % d.luma_sampling
    return int(words[1]), np.fromfile(tmp_path / "out.bin", np.uint8).reshape(d.H, d.W + pad)


def files(layout):
    return [("1x1", gc.write(cases.image(1, 1, "noise"), layout)),
            ("37x53-noise", gc.write(cases.image(37, 53, "noise"), layout)),
            ("33x130-smooth", gc.write(cases.image(33, 130, "smooth"), layout)),
            ("66x257-noise", gc.write(cases.image(66, 257, "noise"), layout)),      # crosses both seams of the 64 x 128 tile
            ("66x3-noise", gc.write(cases.image(66, 3, "noise"), layout))]          # a chroma plane too narrow for libjpeg's filters


@pytest.mark.parametrize("pad", (0, 3))
@pytest.mark.parametrize("layout", gc.LAYOUTS)
def test_gray_planes_equal_the_gray_of_pillow_without_a_sanitizer_report(program, tmp_path, layout, pad):
    for name, data in files(layout):
        d = jpegdec.parse(data, samplings=jpegdec.DEVICE_SAMPLINGS)
        assert d.C == (1 if layout == "gray" else 3)
        status, got = run(program, tmp_path, data, pad)
        assert status == 0, (layout, name)
        assert np.array_equal(got[:, :d.W], gc.expected_gray(data)), (layout, name)
        assert np.all(got[:, d.W:] == 0xA5), (layout, name)                        # the padding of a row is not written
