"""The device JPEG scans with per-image optimal Huffman tables (gs360_jpeg_scan_opt_u8, gs360_jpeg_huff_tables; csrc/gs360_jpeg.hip)
against the restatement of "JPG-SPEC v1, optimal tables" (tests/jpegopt_np.py): every scan, every length and the 4 x 272 table bytes of
every image byte for byte, with a 0xA5 guard behind every buffer the device writes."""
import io

import numpy as np
import pytest

import gs360
from gs360 import jpegenc

import jpegenc_cases as cases
import jpegenc_np as ref
import jpegopt_np as opt

pytestmark = pytest.mark.gpu

GUARD = 64
TB = 4 * opt.TABLE_BYTES


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
        "7x1028": ref.noise_image(7, 1028, 3, seed=5),
        "130x6": ref.noise_image(130, 6, 3, seed=6),
        "16x600 gray": ref.noise_image(16, 600, 1, seed=7),
    }


IMAGES = _images()
_REF = {}


def want(name, quality, restart, image=None):
    """-> (scan, the image's 4 x 272 table bytes) of the restatement, computed once"""
    key = (name, quality, restart)
    if key not in _REF:
        scan, tables = opt.scan_optimal(IMAGES[name] if image is None else image, quality, restart)
        _REF[key] = (scan, b"".join(opt.table_bytes(t) for t in tables))
    return _REF[key]


def run_scans(ctx, images, quality, restart, pad=0, caps=None, slot=0):
    """-> [(length, the out buffer's bytes with its guard, the image's table bytes)] of ONE gs360_jpeg_scan_opt_u8 call; rows padded by
    `pad` bytes.  The guards behind the lengths and the tables are checked here."""
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
        n = len(jobs)
        d_len, d_tab = ctx.alloc(8 * n + GUARD), ctx.alloc(TB * n + GUARD)
        bufs += [d_len, d_tab]
        ctx.memset(d_len, 0xA5, slot)
        ctx.memset(d_tab, 0xA5, slot)
        ctx.jpeg_scan_opt_dev(jobs, d_len, d_tab, quality=quality, restart=restart, slot=slot)
        raw_len = ctx.download(d_len, (8 * n + GUARD,), np.uint8, slot)
        raw_tab = ctx.download(d_tab, (TB * n + GUARD,), np.uint8, slot)
        assert np.all(raw_len[8 * n:] == 0xA5) and np.all(raw_tab[TB * n:] == 0xA5)
        lengths = raw_len[:8 * n].view(np.uint64)
        return [(int(ln), ctx.download(j[5], (j[6] + GUARD,), np.uint8, slot), raw_tab[k * TB:(k + 1) * TB].tobytes())
                for k, (ln, j) in enumerate(zip(lengths, jobs))]
    finally:
        for b in bufs:
            ctx.free(b)


def first_table_difference(got, wanted):
    for t, tname in enumerate(("DC0", "AC0", "DC1", "AC1")):
        g, w = got[t * 272:(t + 1) * 272], wanted[t * 272:(t + 1) * 272]
        if g != w:
            at = next(i for i in range(272) if g[i] != w[i])
            return f"table {tname} differs at byte {at}: BITS {list(g[:16])} against {list(w[:16])}"
    return "tables equal"


def check(name, result, wanted):
    n, data, tables = result
    scan, wtab = wanted
    assert tables == wtab, (name, first_table_difference(tables, wtab))
    assert n == len(scan), name
    assert data[:n].tobytes() == scan, name
    assert np.all(data[-GUARD:] == 0xA5), name


@pytest.mark.parametrize("restart", [1, 4, 8, 65535])
@pytest.mark.parametrize("quality", [100, 95, 75, 1])
def test_every_shape_in_one_call_matches_the_restatement(ctx, quality, restart):
    names = list(IMAGES)
    got = run_scans(ctx, [IMAGES[n] for n in names], quality, restart)
    for name, res in zip(names, got):
        print(f"{name} q={quality} Ri={restart}: {res[0]} bytes (restatement {len(want(name, quality, restart)[0])})")
        check(name, res, want(name, quality, restart))
        if IMAGES[name].ndim == 2:
            assert res[2][2 * 272:] == bytes(2 * 272), name           # gray: no chroma tables


def test_the_speckle_image_goes_through_the_length_limiter(ctx):
    img = opt.speckle_image()
    (res,) = run_scans(ctx, [img], 100, 8)
    check("speckle", res, want("speckle", 100, 8, img))


@pytest.mark.parametrize("group", ["sweep", "fat block"])
def test_the_longest_tables_and_words(ctx, group):
    """the symbol sweep at quality 100 (about 160 symbols per AC table: the longest HUFFVALs) and the fat block (the longest words)"""
    if group == "sweep":
        _g, quality, restart, items = next(g for g in cases.groups() if g[0] == "sweep" and g[1] == 100)
    else:
        quality, restart, items = 100, 8, [("fat block", cases.fat_block_image())]
    got = run_scans(ctx, [a for _n, a in items], quality, restart)
    for (name, a), res in zip(items, got):
        w = want(name, quality, restart, a)
        print(name, "symbols per table:", [sum(w[1][t * 272:t * 272 + 16]) for t in range(4)])
        check(name, res, w)


def test_the_table_builder_alone(ctx):
    """twelve tables in one gs360_jpeg_huff_tables call: the synthetic histograms, an all-zero one and the speckle image's four"""
    hists = list(opt.synthetic_histograms().values()) + [[0] * 256]
    hists += opt.symbol_hist(ref.coefficients(opt.speckle_image(), 100), 8)
    assert len(hists) == 12
    h = np.array(hists, np.uint32)
    d_h, d_t = ctx.to_device(h.view(np.uint8).reshape(-1)), ctx.alloc(12 * 272 + GUARD)
    try:
        ctx.memset(d_t, 0xA5, 0)
        ctx.jpeg_huff_tables_dev(d_h, 12, d_t)
        got = ctx.download(d_t, (12 * 272 + GUARD,), np.uint8, 0)
    finally:
        ctx.free(d_h)
        ctx.free(d_t)
    assert np.all(got[12 * 272:] == 0xA5)
    for k, hist in enumerate(hists):
        wtab = opt.table_bytes(opt.optimal_table(hist))
        g = got[k * 272:(k + 1) * 272].tobytes()
        assert g == wtab, (k, list(g[:16]), list(wtab[:16]))
    assert got[7 * 272:8 * 272].tobytes() == bytes(272)               # the all-zero histogram


def test_split_batches_slots_and_padded_rows_give_identical_bytes(ctx):
    names = list(IMAGES) * 2                 # 20 jobs: more than one launch batch, so the second batch's lengths and tables offsets
    a = run_scans(ctx, [IMAGES[n] for n in names], 75, 8)
    b = run_scans(ctx, [IMAGES[n] for n in names], 75, 8, slot=1)
    for name, ra, rb in zip(names, a, b):
        check(name, ra, want(name, 75, 8))
        assert ra[0] == rb[0] and ra[2] == rb[2] and ra[1].tobytes() == rb[1].tobytes(), name
    names = ["37x53 noise", "33x41 gray", "7x1028", "9x17 flat"]
    for pad in (1, 5):                      # rows that start on every byte alignment
        got = run_scans(ctx, [IMAGES[n] for n in names], 95, 4, pad=pad)
        for name, res in zip(names, got):
            check(name, res, want(name, 95, 4))


def test_the_count_pass_split_does_not_change_the_bytes(ctx):
    """context option jpeg_count_waves: one wavefront per image, and more wavefronts than the image has restart intervals"""
    names = ["75x100 photo", "16x600 gray", "7x1028", "1x1"]
    for waves in (1, 3, 4096):
        with ctx.options(jpeg_count_waves=waves):
            got = run_scans(ctx, [IMAGES[n] for n in names], 95, 4)
        for name, res in zip(names, got):
            check(name, res, want(name, 95, 4))


def test_a_capacity_one_byte_short_reports_overflow_and_still_writes_the_tables(ctx):
    names = ["37x53 noise", "75x100 photo", "33x41 gray"]
    wants = [want(n, 100, 8) for n in names]
    caps = [len(wants[0][0]), len(wants[1][0]) - 1, len(wants[2][0]) + 3]      # exact fit, one short, roomy
    got = run_scans(ctx, [IMAGES[n] for n in names], 100, 8, caps=caps)
    check(names[0], got[0], wants[0])
    assert got[1][0] == gs360.capi.JPEG_OVERFLOW
    assert np.all(got[1][1] == 0xA5)                                   # buffer and guard untouched
    assert got[1][2] == wants[1][1]                                    # the tables do not depend on the capacity
    check(names[2], got[2], wants[2])


def test_encode_device_optimal_files_equal_the_restatement_and_decode_in_pillow(ctx):
    Image = pytest.importorskip("PIL.Image")
    names = ["75x100 photo", "33x41 gray", "1x1"]
    files = jpegenc.encode_device(ctx, [IMAGES[n] for n in names], quality=95, restart=8, huffman="optimal")
    std = jpegenc.encode_device(ctx, [IMAGES[n] for n in names], quality=95, restart=8, huffman="standard")
    for name, f, s in zip(names, files, std):
        assert f == opt.encode_optimal(IMAGES[name], 95, 8), name
        assert s == ref.encode(IMAGES[name], 95, 8), name              # the standard mode in the same process: unchanged
        assert len(f) < len(s), name
        a, b = np.asarray(Image.open(io.BytesIO(f))), np.asarray(Image.open(io.BytesIO(s)))
        assert a.shape == IMAGES[name].shape and np.array_equal(a, b), name
    with pytest.raises(ValueError):
        jpegenc.encode_device(ctx, [IMAGES["1x1"]], huffman="best")


def test_argument_errors(ctx):
    src = ctx.to_device(np.zeros((8, 8, 4), np.uint8))
    out, d_len, d_tab = ctx.alloc(4096), ctx.alloc(8), ctx.alloc(TB)
    try:
        for job, q, ri, code in [((src, 8, 8, 4, 0, out, 4096), 90, 8, -4), ((src, 8, 8, 2, 0, out, 4096), 90, 8, -4),
                                 ((src, 8, 8, 3, 0, out, 4096), 0, 8, -1), ((src, 8, 8, 3, 0, out, 4096), 101, 8, -1),
                                 ((src, 8, 8, 3, 0, out, 4096), 90, 0, -1), ((src, 8, 8, 3, 0, out, 4096), 90, 65536, -1),
                                 ((src, 0, 8, 3, 0, out, 4096), 90, 8, -1), ((src, 8, 65536, 3, 0, out, 4096), 90, 8, -1),
                                 ((src, 8, 8, 3, 23, out, 4096), 90, 8, -1)]:
            with pytest.raises(gs360.Gs360Error) as e:
                ctx.jpeg_scan_opt_dev([job], d_len, d_tab, quality=q, restart=ri)
            assert e.value.code == code, (job[1:5], q, ri)
        with pytest.raises(gs360.Gs360Error) as e:
            ctx.jpeg_scan_opt_dev([(src, 8, 8, 3, 0, out, 4096)], d_len, None, quality=90, restart=8)       # NULL tables_dev
        assert e.value.code == -1
        L = ctx.L
        assert L.gs360_jpeg_huff_tables(ctx.handle, None, 1, d_tab.ptr, 0) == -1
        assert L.gs360_jpeg_huff_tables(ctx.handle, d_len.ptr, 1, None, 0) == -1
        assert L.gs360_jpeg_huff_tables(ctx.handle, d_len.ptr, -1, d_tab.ptr, 0) == -1
        assert L.gs360_jpeg_huff_tables(ctx.handle, None, 0, None, 0) == 0
    finally:
        for b in (src, out, d_len, d_tab):
            ctx.free(b)
