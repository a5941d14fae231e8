"""The device JPEG scans (gs360_jpeg_scan_u8, csrc/gs360_jpeg.hip) against the NumPy restatement of JPG-SPEC v1 (tests/jpegenc_np.py):
every scan and every length byte for byte."""
import io

import numpy as np
import pytest

import gs360
from gs360 import jpegenc

import jpegenc_np as ref
import jpegopt_np as opt
from util import CountingPool

pytestmark = pytest.mark.gpu

GUARD = 64


def _images():
    photo = ref.photo_image()
    return {
        "1x1": np.full((1, 1, 3), 200, np.uint8),
        "8x8": np.full((8, 8, 3), 17, np.uint8),
        "9x17 flat": np.full((9, 17, 3), (255, 0, 128), np.uint8),
        "37x53 noise": ref.noise_image(),
        "75x100 photo": photo,
        "24x40 checker": ref.checker_image(),
        "33x41 gray": ref.gray_of(photo)[:33, :41],
        "7x1028": ref.noise_image(7, 1028, 3, seed=5),          # more than one 256-column strip per block row, a partial last block
        "130x6": ref.noise_image(130, 6, 3, seed=6),
        "16x600 gray": ref.noise_image(16, 600, 1, seed=7),     # gray across strips
    }


IMAGES = _images()
_REF = {}


def want_scan(name, quality, restart):
    key = (name, quality, restart)
    if key not in _REF:
        _REF[key] = ref.scan(IMAGES[name], quality, restart)
    return _REF[key]


def run_scans(ctx, images, quality, restart, pad=0, caps=None, slot=0):
    """-> [(length, the out buffer's bytes with its guard)] of ONE gs360_jpeg_scan_u8 call; rows padded by `pad` bytes"""
    bufs, jobs = [], []
    try:
        for k, a in enumerate(images):
            a3 = a if a.ndim == 3 else a[:, :, None]
            H, W, C = a3.shape
            stride = W * C + pad
            rows = np.full((H, stride), 0xEE, np.uint8)
            rows[:, :W * C] = a3.reshape(H, W * C)
            src = ctx.to_device(rows)
            cap = jpegenc.scan_bound(H, W, C, restart) if caps is None else caps[k]
            out = ctx.alloc(cap + GUARD)
            ctx.memset(out, 0xA5, slot)       # asynchronous: on the stream the scan kernels follow on
            bufs += [src, out]
            jobs.append((src, H, W, C, stride if pad else 0, out, cap))
        d_len = ctx.alloc(8 * len(jobs))
        bufs.append(d_len)
        ctx.jpeg_scan_dev(jobs, d_len, quality=quality, restart=restart, slot=slot)
        lengths = ctx.download(d_len, (len(jobs),), np.uint64, slot)
        return [(int(n), ctx.download(j[5], (j[6] + GUARD,), np.uint8, slot)) for n, j in zip(lengths, jobs)]
    finally:
        for b in bufs:
            ctx.free(b)


@pytest.mark.parametrize("restart", [1, 4, 8, 65535])
@pytest.mark.parametrize("quality", [100, 95, 75, 1])
def test_every_shape_in_one_call_matches_the_restatement(ctx, quality, restart):
    names = list(IMAGES)
    got = run_scans(ctx, [IMAGES[n] for n in names], quality, restart)
    for name, (n, data) in zip(names, got):
        want = want_scan(name, quality, restart)
        print(f"{name} q={quality} Ri={restart}: {n} bytes (restatement {len(want)})")
        assert n == len(want), name
        assert data[:n].tobytes() == want, name
        assert np.all(data[-GUARD:] == 0xA5), name


def test_padded_rows_give_the_same_scans(ctx):
    names = ["37x53 noise", "33x41 gray", "7x1028", "9x17 flat"]
    for pad in (1, 5):                      # rows that start on every byte alignment
        got = run_scans(ctx, [IMAGES[n] for n in names], 95, 4, pad=pad)
        for name, (n, data) in zip(names, got):
            assert data[:n].tobytes() == want_scan(name, 95, 4), (name, pad)


def test_a_capacity_one_byte_short_reports_overflow_and_writes_nothing(ctx):
    names = ["37x53 noise", "75x100 photo", "33x41 gray"]
    wants = [want_scan(n, 100, 8) for n in names]
    caps = [len(wants[0]), len(wants[1]) - 1, len(wants[2]) + 3]      # exact fit, one short, roomy
    got = run_scans(ctx, [IMAGES[n] for n in names], 100, 8, caps=caps)
    assert got[0][0] == len(wants[0]) and got[0][1][:caps[0]].tobytes() == wants[0]
    assert got[1][0] == gs360.capi.JPEG_OVERFLOW
    assert np.all(got[1][1] == 0xA5)                                   # buffer and guard untouched
    assert got[2][0] == len(wants[2]) and got[2][1][:len(wants[2])].tobytes() == wants[2]
    for _n, data in got:
        assert np.all(data[-GUARD:] == 0xA5)


def test_two_calls_and_a_split_batch_give_identical_bytes(ctx):
    names = list(IMAGES) * 2                 # 20 jobs: more than one launch batch
    a = run_scans(ctx, [IMAGES[n] for n in names], 75, 8)
    b = run_scans(ctx, [IMAGES[n] for n in names], 75, 8, slot=1)
    for name, (na, da), (nb, db) in zip(names, a, b):
        assert na == nb == len(want_scan(name, 75, 8)), name
        assert da[:na].tobytes() == db[:nb].tobytes() == want_scan(name, 75, 8), name


def test_encode_device_files_equal_the_restatement_and_decode_in_pillow(ctx):
    Image = pytest.importorskip("PIL.Image")
    names = ["75x100 photo", "33x41 gray", "1x1"]
    files = jpegenc.encode_device(ctx, [IMAGES[n] for n in names], quality=95, restart=8)
    d_img = ctx.to_device(IMAGES["37x53 noise"])
    files += jpegenc.encode_device(ctx, [(d_img, 37, 53, 3)])           # a device buffer, the defaults: quality 100, Ri 8
    ctx.free(d_img)
    wants = [ref.encode(IMAGES[n], 95, 8) for n in names] + [ref.encode(IMAGES["37x53 noise"], 100, 8)]
    for name, f, w in zip(names + ["37x53 noise"], files, wants):
        assert f == w, name
        im = np.asarray(Image.open(io.BytesIO(f)))
        assert im.shape == IMAGES[name].shape, name
        err = np.abs(im.astype(int) - IMAGES[name].astype(int)).mean()
        assert err < 6.0, (name, err)                                   # the picture, not noise (quality >= 95)


# ---- the re-code path of jpegenc.scan_items under pool allocators, as the engine configures it -----------------------------------
def _recode_images():
    """Gray noise, a photo and RGB noise, and a 3 x 3 gray image.  With optimal tables at quality 95 none of the first three needs more than its
    raw size (restated scans of 803 / 863 / 4513 bytes against 960 / 3072 / 5883), so without a fourth nothing would be coded again in
    that mode; an image below one block does in every mode (45 to 79 bytes against 9)."""
    return [ref.noise_image(24, 40, 1), ref.photo_image(32, 32), ref.noise_image(37, 53, 3), ref.noise_image(3, 3, 1)]


_RECODE_REF = {}


def recode_reference(huffman, quality):
    """-> ([whole file], {indices whose restated scan is longer than H * W * C}) of _recode_images(), computed once per mode"""
    key = (huffman, quality)
    if key not in _RECODE_REF:
        files, longer = [], set()
        for i, im in enumerate(_recode_images()):
            H, W = im.shape[:2]
            C = 1 if im.ndim == 2 else 3
            if huffman == "optimal":
                scan, tables = opt.scan_optimal(im, quality, jpegenc.RESTART)
                head = opt.header_optimal(H, W, C, quality, jpegenc.RESTART, tables)
            else:
                scan, head = ref.scan(im, quality, jpegenc.RESTART), ref.header(H, W, C, quality, jpegenc.RESTART)
            files.append(head + scan + b"\xff\xd9")
            if len(scan) > im.size:
                longer.add(i)
        _RECODE_REF[key] = (files, longer)
    return _RECODE_REF[key]


@pytest.mark.parametrize("quality", [100, 95])
@pytest.mark.parametrize("huffman", ["standard", "optimal"])
def test_scans_past_their_raw_size_are_coded_again_under_pool_allocators(ctx, huffman, quality):
    """jpegenc.scan_items as Engine._encode_views calls it (4:4:4, jpegenc.RESTART, raw-size first capacities, taking and giving
    callables over a pool): the files equal the restatement's, exactly the items whose restated scan exceeds H * W * C were coded
    again, and everything taken but the returned scan buffers went back."""
    images = _recode_images()
    wants, longer = recode_reference(huffman, quality)
    print(f"{huffman} q={quality}: restated scans longer than the raw size: {sorted(longer)} of {len(images)}")
    assert 0 < len(longer) < len(images)             # both branches run in every parametrisation
    pool = CountingPool(ctx)
    srcs = [ctx.to_device(im) for im in images]
    items = [(d, im.shape[0], im.shape[1], 1 if im.ndim == 2 else 3) for d, im in zip(srcs, images)]
    try:
        with ctx.slot_locks[0]:
            scans = jpegenc.scan_items(ctx, items, pool.take, pool.give, quality, jpegenc.RESTART, 0, huffman)
        assert pool.takes == pool.gives + len(scans)
        assert pool.takes == len(images) + (2 if huffman == "optimal" else 1) + len(longer)
        recoded = {i for i, ((d, _n, _t), im) in enumerate(zip(scans, images)) if d.nbytes != im.size}
        assert recoded == longer
        for i, ((d, n, tab), (_s, H, W, C)) in enumerate(zip(scans, items)):
            assert d.nbytes == (jpegenc.scan_bound(H, W, C, jpegenc.RESTART) if i in longer else H * W * C), i
            assert (tab is None) == (huffman == "standard"), i
            got = jpegenc.header(H, W, C, quality, jpegenc.RESTART, tab) + ctx.download(d, (n,), np.uint8).tobytes() + jpegenc.EOI
            assert got == wants[i], i
        for d, _n, _t in scans:
            pool.give(d)
        assert pool.takes == pool.gives
    finally:
        pool.close()
        for d in srcs:
            ctx.free(d)


@pytest.mark.parametrize("huffman", ["standard", "optimal"])
def test_the_engine_replaces_the_pinned_block_of_exactly_the_views_coded_again(huffman):
    """Engine._encode_views itself, without a render: a device state of its own, hand-made view outputs and pinned blocks.  Its views
    share one channel count, so the RGB images of the set at quality 100 (the noise is coded again, the photo is not)."""
    from gs360 import engine
    wants, longer = recode_reference(huffman, 100)
    pick = [i for i, im in enumerate(_recode_images()) if im.ndim == 3]
    images = [_recode_images()[i] for i in pick]
    assert 0 < len(longer & set(pick)) < len(pick)
    st = engine._DeviceState(0)
    try:
        d_out = [st.ctx.to_device(im) for im in images]
        blocks = [st.ctx.pinned(im.size) for im in images]
        h_out = list(blocks)
        with st.ctx.slot_locks[0]:
            out = engine.Engine._encode_views(None, st, st.ctx, 0, d_out, h_out, [im.shape[:2] for im in images], 3, (100, huffman))
        for k, i in enumerate(pick):
            assert bytes(out[k].header) + out[k].scan.tobytes() + jpegenc.EOI == wants[i], i
            assert (h_out[k] is not blocks[k]) == (i in longer), i
            assert h_out[k].nbytes >= out[k].scan.size and (h_out[k].nbytes > blocks[k].nbytes) == (i in longer), i
        assert st.stats["jpeg_device_images"] == len(pick) and st.stats["jpeg_device_bytes"] == sum(len(wants[i]) for i in pick)
        assert sum(len(v) for v in st.dev_pool.values()) == len(pick) + (2 if huffman == "optimal" else 1) + len(longer & set(pick))
    finally:
        st.ctx.close()


def test_argument_errors(ctx):
    src = ctx.to_device(np.zeros((8, 8, 4), np.uint8))
    out, d_len = ctx.alloc(4096), ctx.alloc(8)
    try:
        for job, q, ri, code in [((src, 8, 8, 4, 0, out, 4096), 90, 8, -4), ((src, 8, 8, 2, 0, out, 4096), 90, 8, -4),
                                 ((src, 8, 8, 3, 0, out, 4096), 0, 8, -1), ((src, 8, 8, 3, 0, out, 4096), 101, 8, -1),
                                 ((src, 8, 8, 3, 0, out, 4096), 90, 0, -1), ((src, 8, 8, 3, 0, out, 4096), 90, 65536, -1),
                                 ((src, 0, 8, 3, 0, out, 4096), 90, 8, -1), ((src, 8, 65536, 3, 0, out, 4096), 90, 8, -1),
                                 ((src, 8, 8, 3, 23, out, 4096), 90, 8, -1)]:
            with pytest.raises(gs360.Gs360Error) as e:
                ctx.jpeg_scan_dev([job], d_len, quality=q, restart=ri)
            assert e.value.code == code, (job[1:5], q, ri)
        with pytest.raises(gs360.Gs360Error) as e:
            jpegenc.scan_bound(8, 8, 4)
        assert e.value.code == -4
        assert jpegenc.scan_bound(9, 17, 3, 4) == 2 * 3 * 3 * 416 + 2 * 3
    finally:
        for b in (src, out, d_len):
            ctx.free(b)
