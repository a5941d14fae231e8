"""The device JPEG decoder's bounds for 4:2:2, 4:4:0 and 4:1:1 files, checked on the CPU: tests/tools/jpegdec_hostcheck.hip steps the
kernels' own stage functions (csrc/gs360_jpegdec.hip) lane by lane on the host, built with AddressSanitizer and
UndefinedBehaviorSanitizer and with every buffer at its exact size, the scratch by the layout of the file's own sampling.  Valid files
must give Pillow's pixels with status 0; truncated and corrupted scans must give a status (or the restatement's pixels) and, like the
valid ones, no sanitizer report.  A stand-alone program: nothing is loaded into python."""
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
import jpegsamp_np as samp  # noqa: E402

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
MODES = tuple(samp.SAMPLINGS)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc to build the host check with")
    if os.environ.get("LD_PRELOAD"):
        pytest.skip("a preloaded library and a sanitized program do not go together")
    exe = tmp_path_factory.mktemp("hostcheck") / "jpegdec_hostcheck"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "tools" / "jpegdec_hostcheck.hip")],
                   check=True, capture_output=True, timeout=600)
    return exe


def run(program, tmp_path, data):
    """-> (status, pixels H x W x C) of the host-stepped decoder on one file"""
    d = jpegdec.parse(data, samplings=jpegdec.DEVICE_SAMPLINGS)
    seg, n_sub = jpegdec.segment_table(d)
    head = struct.pack("16i", d.H, d.W, d.C, d.subsampling, d.restart, d.scan_len, seg.shape[0], n_sub, *([0] * 8))
    sel = bytes((d.comp_tq + [0] * 4)[:4] + (d.comp_td + [0] * 4)[:4] + (d.comp_ta + [0] * 4)[:4])
    (tmp_path / "in.bin").write_bytes(head + sel + data[d.scan_off:d.scan_off + d.scan_len] + seg.tobytes() + d.huff.tobytes() + d.quant.tobytes())
    r = subprocess.run([str(program), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    words = r.stdout.split()
    hs, vs = d.luma_sampling
    assert words[words.index("sampling") + 1] == "%dx%d" % (hs, vs) and int(words[words.index("bpm") + 1]) == d.blocks_per_mcu
    return int(words[1]), np.fromfile(tmp_path / "out.bin", np.uint8).reshape(d.H, d.W, d.C)


def files(mode):
    hs, vs = samp.SAMPLINGS[mode]
    out = [("37x53-noise", samp.write(cases.image(37, 53, "noise"), hs, vs, 90, 0)),
           ("33x130-smooth", samp.write(cases.image(33, 130, "smooth"), hs, vs, 90, 0)),
           ("1x1", samp.write(cases.image(1, 1, "noise"), hs, vs, 90, 0)),
           ("160x224-noise-q100", samp.write(cases.image(160, 224, "noise", seed=5), hs, vs, 100, 0))]      # several entropy workgroups
    out += [("ri%d" % ri, samp.write(cases.image(100, 150, "noise", seed=3), hs, vs, 95, ri)) for ri in (1, 7)]
    if mode == "4:2:2":
        out.append(("pillow", cases.encode(cases.image(37, 53, "noise"), quality=90, subsampling=1)))
    return out


@pytest.mark.parametrize("mode", MODES)
def test_valid_files_equal_pillow_without_a_sanitizer_report(program, tmp_path, mode):
    for name, data in files(mode):
        if name.startswith("160x224"):
            d = jpegdec.parse(data, samplings=jpegdec.DEVICE_SAMPLINGS)
            assert jpegdec.segment_table(d)[1] > jpegdec.subseqs_per_workgroup(), name
        status, got = run(program, tmp_path, data)
        assert status == 0 and np.array_equal(got, cases.pillow(data)), (mode, name)


@pytest.mark.parametrize("mode", MODES)
def test_truncated_and_corrupt_scans_stay_in_bounds(program, tmp_path, mode):
    hs, vs = samp.SAMPLINGS[mode]
    data = samp.write(cases.image(64, 64, "noise"), hs, vs, 90, 0)
    d = jpegdec.parse(data, samplings=jpegdec.DEVICE_SAMPLINGS)
    status, _ = run(program, tmp_path, data[:d.scan_off + d.scan_len // 2] + b"\xff\xd9")
    assert status != 0
    tried = 0
    for seed in range(8):
        bad = bytearray(data)
        at = d.scan_off + d.scan_len // 2
        bad[at:at + 64] = np.random.default_rng(seed).integers(0, 256, 64, dtype=np.uint8).tobytes()
        try:
            jpegdec.parse(bytes(bad), samplings=jpegdec.DEVICE_SAMPLINGS)
        except jpegdec.Unsupported:
            continue                     # (a marker among the random bytes: the host keeps the file)
        tried += 1
        status, got = run(program, tmp_path, bytes(bad))
        if status == 0:
            assert np.array_equal(got, samp.decode(bytes(bad)))
    assert tried >= 4
