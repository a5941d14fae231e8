"""-m gpu: the gray output mode of the device JPEG decoder (gs360_jpeg_decode_gray_u8 through gs360.jpegdec).
Every plane is compared byte for byte with FS-SPEC's gray of Pillow's pixels for the same file, (4899 R + 9617 G + 1868 B + 8192) >> 14
(Pillow's L array for a gray file), status 0: no tolerance anywhere."""
import numpy as np
import pytest

pytest.importorskip("PIL.Image")

import gs360  # noqa: E402
from gs360 import jpegdec  # noqa: E402

import jpegdec_cases as cases  # noqa: E402
import jpeggray_cases as gc  # noqa: E402
import jpegsamp_cases as sc  # noqa: E402
import jpegsamp_np as samp  # noqa: E402

pytestmark = pytest.mark.gpu

WG = jpegdec.subseqs_per_workgroup()
GUARD = 256
WIDE = jpegdec.DEVICE_SAMPLINGS


@pytest.fixture(scope="module")
def ctx():
    with gs360.Context(device=0, n_slots=2) as c:
        yield c


def gray_to_host(ctx, datas, slot=0):
    """-> ([H x W plane or None], [status]) of one gray decode call"""
    out, codes = [], []
    for r in jpegdec.decode_device(ctx, datas, slot, gray=True):
        codes.append(r.status)
        if r.buf is None:
            out.append(None)
            continue
        H, W, C = r.shape
        assert C == 1 and r.stride == W
        out.append(ctx.download(r.buf, (H, W), np.uint8, slot))
        ctx.free(r.buf)
    return out, codes


def check(ctx, files, slot=0):
    """files: [(name, bytes)] -> gray decode calls of up to 64 files; every plane equals the expected gray with status 0"""
    for at in range(0, len(files), 64):
        part = files[at:at + 64]
        got, status = gray_to_host(ctx, [d for _n, d in part], slot)
        for (name, data), a, code in zip(part, got, status):
            assert code == 0, (name, code)
            assert np.array_equal(a, gc.expected_gray(data)), name


def test_pillow_matrix_equals_expected_gray(ctx):
    files = cases.matrix_once()
    assert len(files) == 228
    check(ctx, files)


@pytest.mark.parametrize("mode", sc.MODES)
def test_written_matrix_equals_expected_gray(ctx, mode):
    files = sc.written(mode)
    assert len(files) == 78 and {n.split("-")[1] for n, _ in files} >= {"1x1", "66x257"}
    check(ctx, files)


def test_gray_is_not_the_luma_plane(ctx):
    """the condition against a vacuous comparison: on a colourful file the expected gray differs from the file's Y plane (what libjpeg
    returns when asked for gray output), and the device gives the former"""
    import io
    from PIL import Image
    data = cases.encode(cases.image(37, 53, "noise"), quality=90, subsampling=0)
    im = Image.open(io.BytesIO(data))
    im.draft("L", im.size)
    luma = np.asarray(im)
    assert luma.shape == (37, 53) and not np.array_equal(gc.expected_gray(data), luma)
    check(ctx, [("colourful", data)])


def test_one_call_mixes_a_gray_file_and_the_five_colour_layouts(ctx):
    files = [("gray", gc.write(cases.image(48, 80, "noise", seed=4), "gray")),
             ("444", gc.write(cases.image(120, 200, "noise", seed=1), "4:4:4", 95)),
             ("420", gc.write(cases.image(33, 130, "smooth"), "4:2:0", 30)),
             ("422", gc.write(cases.image(130, 33, "noise", seed=2), "4:2:2")),
             ("440", gc.write(cases.image(65, 255, "noise", seed=3), "4:4:0", 92, 5)),
             ("411", gc.write(cases.image(66, 257, "smooth"), "4:1:1", 75))]
    ds = [jpegdec.parse(d, samplings=WIDE) for _n, d in files]
    assert [(d.C, d.subsampling) for d in ds] == [(1, 0), (3, 0), (3, 2), (3, 1), (3, 3), (3, 4)]
    got, status = gray_to_host(ctx, [d for _n, d in files], slot=1)
    assert status == [0] * 6
    for (name, data), a in zip(files, got):
        assert np.array_equal(a, gc.expected_gray(data)), name


@pytest.mark.parametrize("layout", ("4:2:0", "4:4:4"))
@pytest.mark.parametrize("pad", (0, 1, 3))
def test_padded_planes_leave_pad_and_guard_alone(ctx, layout, pad):
    """widths around the store's alignment and the tile's seam, at a height past one tile: the image bytes are the expected gray, and
    every pad byte of every row and every guard byte behind the plane and behind the scratch still hold 0xA5"""
    widths = (1, 2, 3, 5, 127, 129, 257)
    datas = [gc.write(cases.image(66, w, "noise", seed=w), layout) for w in widths]
    batch = jpegdec.Batch(ctx, datas, pad=pad, guard=GUARD, gray=True)
    try:
        assert not batch.refused, batch.refused
        batch.run()
        assert batch.status() == [0] * len(widths)
        for (_k, d, b_out, b_scr, nscr, stride), data, w in zip(batch.items, datas, widths):
            assert (d.H, d.W, stride) == (66, w, w + pad)
            out = ctx.download(b_out, (66 * stride + GUARD,), np.uint8)
            scr = ctx.download(b_scr, (nscr + GUARD,), np.uint8)
            rows = out[:66 * stride].reshape(66, stride)
            assert np.array_equal(rows[:, :w], gc.expected_gray(data)), (layout, w, pad)
            assert np.all(rows[:, w:] == 0xA5) and np.all(out[66 * stride:] == 0xA5) and np.all(scr[nscr:] == 0xA5), (layout, w, pad)
    finally:
        batch.close()


def test_scan_across_more_than_two_entropy_workgroups(ctx):
    """256 x 384 noise at quality 100 without restarts, as tests/test_jpegsamp_gpu.py builds it: the shared stages feed the gray one"""
    files = []
    for mode in sc.MODES:
        hs, vs = samp.SAMPLINGS[mode]
        data = samp.write(cases.image(256, 384, "noise", seed=5), hs, vs, 100, 0)
        d = jpegdec.parse(data, samplings=WIDE)
        assert d.restart == 0 and jpegdec.segment_table(d)[1] > 2 * WG
        files.append(("noise-" + mode, data))
    check(ctx, files)


def test_truncated_scan_gives_a_status_and_no_buffer(ctx):
    data = gc.write(cases.image(64, 64, "noise"), "4:2:0")
    d = jpegdec.parse(data, samplings=WIDE)
    cut = data[:d.scan_off + d.scan_len // 2] + b"\xff\xd9"
    gray = jpegdec.decode_device(ctx, [cut, data], gray=True)
    rgb = jpegdec.decode_device(ctx, [cut, data])
    try:
        assert gray[0].status != 0 and gray[0].buf is None and (gray[0].status, gray[0].reason) == (rgb[0].status, rgb[0].reason)
        assert gray[1].status == 0 and gray[1].shape == (64, 64, 1) and rgb[1].shape == (64, 64, 3)
        assert np.array_equal(ctx.download(gray[1].buf, (64, 64), np.uint8), gc.expected_gray(data))
    finally:
        for r in gray + rgb:
            if r.buf is not None:
                ctx.free(r.buf)
    refused = jpegdec.decode_device(ctx, [b"not a jpeg"], gray=True)[0]
    assert refused.buf is None and refused.status == -1


def test_rgb_entry_point_still_equals_pillow(ctx):
    """the shared code is intact: the same files through gs360_jpeg_decode_u8"""
    files = [(layout, gc.write(cases.image(66, 257, "noise", seed=9), layout)) for layout in gc.LAYOUTS]
    got, status = jpegdec.decode_to_host(ctx, [d for _n, d in files])
    assert status == [0] * len(files)
    for (name, data), a in zip(files, got):
        assert np.array_equal(a, cases.pillow(data)), name
    check(ctx, files)


def test_narrow_files_equal_pillow_in_both_modes(ctx):
    """libjpeg filters a chroma plane subsampled by two along x only when it is more than two samples wide; below that (images up to
    four pixels wide) it replicates on both axes"""
    files = [(f"{layout}-{h}x{w}", gc.write(cases.image(h, w, "noise", seed=w), layout))
             for layout in ("4:2:0", "4:2:2") for h, w in ((66, 1), (66, 2), (66, 3), (66, 4), (66, 5), (4, 4), (3, 3))]
    got, status = jpegdec.decode_to_host(ctx, [d for _n, d in files])
    assert status == [0] * len(files)
    for (name, data), a in zip(files, got):
        assert np.array_equal(a, cases.pillow(data)), name
    check(ctx, files)
