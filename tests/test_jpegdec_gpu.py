"""-m gpu: gs360_jpeg_decode_u8 through gs360.jpegdec (JPD-SPEC v1).  Every comparison is byte for byte with
np.asarray(PIL.Image.open(...)) of the same file, status 0; the cases aim at the entropy stage's seams (subsequence, workgroup and
restart-segment boundaries, stuffed bytes on a boundary), not at pixel counts, and read the subsequence size from the binding."""
import numpy as np
import pytest

pytest.importorskip("PIL.Image")

import gs360  # noqa: E402
from gs360 import capi, jpegdec, jpegenc  # noqa: E402

import jpegdec_cases as cases  # noqa: E402
import jpegdec_np as ref  # noqa: E402

pytestmark = pytest.mark.gpu

SUB = jpegdec.subseq_bytes()
WG = jpegdec.subseqs_per_workgroup()
GUARD = 256


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


def test_matrix_equals_pillow(ctx):
    check(ctx, cases.matrix_once())


def test_scan_across_three_workgroups_without_restarts(ctx):
    """noise at quality 100, no DRI: lanes of one workgroup cannot know their entry states from inside it"""
    for sub in (0, 2):
        data = cases.encode(cases.image(256, 384, "noise", seed=5), quality=100, subsampling=sub)
        d = jpegdec.parse(data)
        assert d.restart == 0 and d.segments.shape[0] == 1
        assert d.scan_len >= 3 * WG * SUB, d.scan_len
        check(ctx, [("noise-s%d" % sub, data)])


def test_many_blocks_per_subsequence(ctx):
    """a constant colour: blocks of a few bits each, more than a hundred complete in one subsequence"""
    for sub in (0, 2):
        data = cases.encode(np.full((256, 384, 3), (77, 150, 201), np.uint8), quality=90, subsampling=sub)
        d = jpegdec.parse(data)
        blocks = d.n_mcu * d.blocks_per_mcu
        assert d.scan_len * 8 / blocks < 8 and blocks / (d.scan_len / SUB) > 100, (d.scan_len, blocks)     # about 5 bits a block
        check(ctx, [("flat-s%d" % sub, data)])


@pytest.mark.parametrize("sub", (0, 2))
def test_segment_edges(ctx, sub):
    """restart intervals of one MCU (segments far shorter than a subsequence), of one MCU row, and of 7 MCUs, which divides neither the
    row nor the MCU count (a short last segment; segments that end inside a subsequence)"""
    a = cases.image(200, 300, "noise", seed=3)
    files = []
    for content, quality in ((a, 95), (cases.image(200, 300, "smooth"), 75)):
        d0 = jpegdec.parse(cases.encode(content, quality=quality, subsampling=sub))
        mh, mw = d0.mcu_grid
        for ri in (1, mw, 7):
            assert ri == 1 or ri == mw or d0.n_mcu % ri
            data = cases.encode(content, quality=quality, subsampling=sub, restart_marker_blocks=ri)
            d = jpegdec.parse(data)
            assert d.restart == ri and d.segments.shape[0] == -(-d.n_mcu // ri)
            lengths = d.segments[:, 1]
            if ri == 1 and quality == 75:
                assert lengths.max() < SUB               # every segment shorter than one subsequence
            assert np.any(lengths % SUB)                     # segments that end mid-subsequence
            files.append(("ri%d-q%d" % (ri, quality), data))
    check(ctx, files)


STUFF_SEED = 5      # searched on the CPU: the scan of this image holds FF 00 pairs astride subsequence boundaries


def test_stuffed_bytes_on_subsequence_boundaries(ctx):
    data = cases.encode(cases.image(256, 384, "noise", seed=STUFF_SEED), quality=100, subsampling=0)
    d = jpegdec.parse(data)
    scan = np.frombuffer(data, np.uint8, d.scan_len, d.scan_off)
    pairs = np.flatnonzero((scan[:-1] == 0xFF) & (scan[1:] == 0x00))
    assert pairs.size >= 50
    astride = pairs[pairs % SUB == SUB - 1]                  # the FF ends a subsequence, the 00 starts the next one
    assert astride.size >= 1
    check(ctx, [("stuffing", data)])


@pytest.mark.parametrize("subsampling", ("4:4:4", "4:2:0"))
def test_round_trip_with_the_device_encoder(ctx, subsampling):
    images = [cases.image(96, 160, "noise", seed=9), cases.image(75, 133, "smooth"), cases.image(64, 64, "noise", gray=True)]
    files = jpegenc.encode_device(ctx, images, quality=92, restart=8, huffman="optimal", subsampling=subsampling)
    check(ctx, [("rt%d" % k, f) for k, f in enumerate(files)])


def test_batch_equals_single_calls(ctx):
    files = [("a", cases.encode(cases.image(120, 200, "noise", seed=1), quality=95, subsampling=2)),
             ("b", cases.encode(cases.image(33, 130, "smooth"), quality=30, subsampling=0, optimize=True)),
             ("c", cases.encode(cases.image(64, 48, "noise", gray=True), quality=90)),
             ("d", cases.encode(cases.image(17, 16, "noise"), quality=100, subsampling=2, restart_marker_blocks=2)),
             ("e", cases.encode(cases.image(256, 384, "noise", seed=2), quality=100, subsampling=0))]
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
        batch.run()
        (status,) = batch.status()
        (_k, d, b_out, b_scr, nscr, stride), = batch.items
        out = ctx.download(b_out, (d.H * stride + GUARD,), np.uint8)
        scr = ctx.download(b_scr, (nscr + GUARD,), np.uint8)
        return status, stride, out, scr[nscr:]
    finally:
        batch.close()


def test_padded_output_pitch(ctx):
    for sub, pad in ((0, 5), (2, 13)):
        data = cases.encode(cases.image(37, 53, "noise"), quality=90, subsampling=sub)
        status, stride, out, guard = run_guarded(ctx, data, pad)
        assert status == 0 and stride == 53 * 3 + pad
        rows = out[:37 * stride].reshape(37, stride)
        assert np.array_equal(rows[:, :53 * 3].reshape(37, 53, 3), cases.pillow(data))
        assert np.all(rows[:, 53 * 3:] == 0xA5) and np.all(out[37 * stride:] == 0xA5) and np.all(guard == 0xA5)


BOUNDS_SEED = 0     # searched on the CPU: the substituted bytes hold no marker, so parse() still accepts the file


@pytest.mark.parametrize("sub", (0, 2))
def test_truncated_and_corrupt_scans_stay_inside_their_buffers(ctx, sub):
    """the error path: a scan cut to half its length reports a status; 64 random bytes mid-scan give a status or the restatement's
    pixels; nothing behind the output or behind the scratch (whose last part is the coefficients) is written"""
    data = cases.encode(cases.image(64, 64, "noise"), quality=90, subsampling=sub)
    d = jpegdec.parse(data)
    cut = data[:d.scan_off + d.scan_len // 2] + b"\xff\xd9"
    status, stride, out, guard = run_guarded(ctx, cut)
    assert status != 0
    assert np.all(out[64 * stride:] == 0xA5) and np.all(guard == 0xA5)
    bad = bytearray(data)
    at = d.scan_off + d.scan_len // 2
    bad[at:at + 64] = np.random.default_rng(BOUNDS_SEED).integers(0, 256, 64, dtype=np.uint8).tobytes()
    bad = bytes(bad)
    jpegdec.parse(bad)
    status, stride, out, guard = run_guarded(ctx, bad)
    assert np.all(out[64 * stride:] == 0xA5) and np.all(guard == 0xA5)
    if status == 0:
        assert np.array_equal(out[:64 * stride].reshape(64, 64, 3), ref.decode(bad))
    # and the untouched file still decodes
    check(ctx, [("intact", data)])


def test_refused_files_are_reported_not_decoded(ctx):
    from PIL import Image
    import io
    f = io.BytesIO()
    Image.fromarray(cases.image(48, 80, "noise")).save(f, "JPEG", progressive=True)
    got, status = jpegdec.decode_to_host(ctx, [f.getvalue(), b"not a jpeg"])
    assert got == [None, None] and status == [-1, -1]
