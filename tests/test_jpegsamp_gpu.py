"""-m gpu: 4:2:2, 4:4:0 and 4:1:1 files through gs360.jpegdec (JPD-SPEC v1).  Every comparison is byte for byte
with np.asarray(PIL.Image.open(...)) of the same file, status 0.  Pillow writes 4:2:2 only; the other files come from the NumPy writer
of tests/jpegsamp_np.py.  The cases aim at the MCU edges (16 x 8, 8 x 16, 32 x 8), at the seams of the 64 x 128 reconstruction tile,
where the chroma halo of the two filtered layouts is read, and at the entropy stage's block cycle (4 or 6 blocks with 2 or 4 of luma)."""
import numpy as np
import pytest

pytest.importorskip("PIL.Image")

import gs360  # noqa: E402
from gs360 import jpegdec  # noqa: E402

import jpegdec_cases as cases  # noqa: E402
import jpegsamp_cases as sc  # noqa: E402
import jpegsamp_np as samp  # noqa: E402

pytestmark = pytest.mark.gpu

SUB = jpegdec.subseq_bytes()
WG = jpegdec.subseqs_per_workgroup()
GUARD = 256
WIDE = jpegdec.DEVICE_SAMPLINGS


@pytest.fixture(scope="module")
def ctx():
    with gs360.Context(device=0, n_slots=2) as c:
        yield c


def check(ctx, files, slot=0):
    """files: [(name, bytes)] -> one decode call; every image equals Pillow's with status 0"""
    got, status = jpegdec.decode_to_host(ctx, [d for _n, d in files], slot)
    for (name, data), a, code in zip(files, got, status):
        assert code == 0, (name, code)
        assert np.array_equal(a, cases.pillow(data)), name


@pytest.mark.parametrize("mode", sc.MODES)
def test_written_matrix_equals_pillow(ctx, mode):
    files = sc.written(mode)
    assert len(files) == 78
    check(ctx, files)


def test_pillow_422_matrix_equals_pillow(ctx):
    files = sc.pillow_422()
    assert len(files) == 234
    check(ctx, files)


def _noise(mode, height):
    hs, vs = samp.SAMPLINGS[mode]
    return samp.write(cases.image(height, 384, "noise", seed=5), hs, vs, 100, 0)


@pytest.mark.parametrize("mode", sc.MODES)
def test_scan_across_more_than_two_workgroups_without_restarts(ctx, mode):
    """noise at quality 100, no DRI: lanes of one workgroup cannot know their entry states from inside it.  256 x 384 gives more than
    2 x 256 subsequences in all three modes (the loop would say otherwise)"""
    height = 256
    data = _noise(mode, height)
    while jpegdec.segment_table(jpegdec.parse(data, samplings=WIDE))[1] <= 2 * WG:
        height += 64
        data = _noise(mode, height)
    d = jpegdec.parse(data, samplings=WIDE)
    n_sub = jpegdec.segment_table(d)[1]
    print(f"{mode}: height {height}, {n_sub} subsequences")
    assert height == 256, height
    assert d.restart == 0 and d.segments.shape[0] == 1 and n_sub > 2 * WG
    check(ctx, [("noise-" + mode, data)])


@pytest.mark.parametrize("mode", sc.MODES)
def test_many_blocks_per_subsequence(ctx, mode):
    """a constant colour: blocks of a few bits each, several MCU cycles complete in one subsequence"""
    hs, vs = samp.SAMPLINGS[mode]
    data = samp.write(np.full((256, 384, 3), (77, 150, 201), np.uint8), hs, vs, 90, 0)
    d = jpegdec.parse(data, samplings=WIDE)
    blocks = d.n_mcu * d.blocks_per_mcu
    assert blocks / (d.scan_len / SUB) > 100, (d.scan_len, blocks)
    check(ctx, [("flat-" + mode, data)])


def test_batch_of_five_layouts_equals_single_calls(ctx):
    files = [("444", cases.encode(cases.image(120, 200, "noise", seed=1), quality=95, subsampling=0)),
             ("420", cases.encode(cases.image(33, 130, "smooth"), quality=30, subsampling=2, optimize=True)),
             ("422", cases.encode(cases.image(130, 33, "noise", seed=2), quality=90, subsampling=1)),
             ("440", samp.write(cases.image(65, 255, "noise", seed=3), 1, 2, 92, 5)),
             ("411", samp.write(cases.image(66, 257, "smooth"), 4, 1, 75, 0))]
    subs = [jpegdec.parse(d, samplings=WIDE).subsampling for _n, d in files]
    assert subs == [0, 2, 1, 3, 4]
    batch, status = jpegdec.decode_to_host(ctx, [d for _n, d in files], slot=1)
    assert status == [0] * 5
    for (name, data), a in zip(files, batch):
        single, code = jpegdec.decode_to_host(ctx, [data])
        assert code == [0] and np.array_equal(single[0], a), name
        assert np.array_equal(a, cases.pillow(data)), name


def run_guarded(ctx, data, pad=0):
    """-> (status, row stride, output bytes with pad and guard, the guard behind the scratch) of one file with 0xA5 in every byte the
    device may not write"""
    batch = jpegdec.Batch(ctx, [data], pad=pad, guard=GUARD)
    try:
        assert not batch.refused, batch.refused
        batch.run()
        (status,) = batch.status()
        (_k, d, b_out, b_scr, nscr, stride), = batch.items
        out = ctx.download(b_out, (d.H * stride + GUARD,), np.uint8)
        scr = ctx.download(b_scr, (nscr + GUARD,), np.uint8)
        return status, stride, out, scr[nscr:]
    finally:
        batch.close()


@pytest.mark.parametrize("mode", sc.MODES)
def test_padded_output_pitch(ctx, mode):
    hs, vs = samp.SAMPLINGS[mode]
    data = samp.write(cases.image(37, 53, "noise"), hs, vs, 90, 0)
    status, stride, out, guard = run_guarded(ctx, data, 11)
    assert status == 0 and stride == 53 * 3 + 11
    rows = out[:37 * stride].reshape(37, stride)
    assert np.array_equal(rows[:, :53 * 3].reshape(37, 53, 3), cases.pillow(data))
    assert np.all(rows[:, 53 * 3:] == 0xA5) and np.all(out[37 * stride:] == 0xA5) and np.all(guard == 0xA5)


@pytest.mark.parametrize("mode", sc.MODES)
def test_truncated_and_corrupt_scans_stay_inside_their_buffers(ctx, mode):
    """the error path: a scan cut to half its length reports a status; 64 random bytes mid-scan (eight seeds, those that put no marker
    into the scan) give a status or the restatement's pixels; nothing behind the output or behind the scratch (whose last part is the
    coefficients) is written, and the intact file still decodes afterwards"""
    hs, vs = samp.SAMPLINGS[mode]
    data = samp.write(cases.image(64, 64, "noise"), hs, vs, 90, 0)
    d = jpegdec.parse(data, samplings=WIDE)
    cut = data[:d.scan_off + d.scan_len // 2] + b"\xff\xd9"
    status, stride, out, guard = run_guarded(ctx, cut)
    assert status != 0
    assert np.all(out[64 * stride:] == 0xA5) and np.all(guard == 0xA5)
    tried = 0
    for seed in range(8):
        bad = bytearray(data)
        at = d.scan_off + d.scan_len // 2
        bad[at:at + 64] = np.random.default_rng(seed).integers(0, 256, 64, dtype=np.uint8).tobytes()
        bad = bytes(bad)
        try:
            jpegdec.parse(bad, samplings=WIDE)
        except jpegdec.Unsupported:
            continue                     # (a marker among the random bytes: the host keeps the file)
        tried += 1
        status, stride, out, guard = run_guarded(ctx, bad)
        assert np.all(out[64 * stride:] == 0xA5) and np.all(guard == 0xA5)
        if status == 0:
            assert np.array_equal(out[:64 * stride].reshape(64, 64, 3), samp.decode(bad))
    assert tried >= 4
    check(ctx, [("intact", data)])
