"""The device JPEG scans with 2 x 2 chroma subsampling (gs360_jpeg_scan_sub_u8 with GS360_JPEG_420, gs360_jpeg_scan_bound_sub;
csrc/gs360_jpeg.hip) against the restatement of "JPG-SPEC v1, 4:2:0" (tests/jpeg420_np.py): every scan, every length and, with
optimal tables, the 4 x 272 table bytes of every image byte for byte, with a 0xA5 guard behind every buffer the device writes."""
import ctypes as ct
import io

import numpy as np
import pytest

import gs360
from gs360 import capi, jpegenc

import jpeg420_np as j420
import jpegopt_np as opt

pytestmark = pytest.mark.gpu

GUARD = 64
TB = 4 * opt.TABLE_BYTES
IMAGES = j420.images()
NAMES = list(IMAGES)
_COEF, _REF = {}, {}


def coefficients(name, quality):
    if (name, quality) not in _COEF:
        _COEF[(name, quality)] = j420.coefficients(IMAGES[name], quality)
    return _COEF[(name, quality)]


def want(name, quality, restart, optimal=False):
    """-> (scan, the image's 4 x 272 table bytes or None) of the restatement, computed once"""
    key = (name, quality, restart, optimal)
    if key not in _REF:
        a = IMAGES[name]
        if optimal:
            if j420.is_gray(a):
                scan, tables = j420.scan_optimal(a, quality, restart)
            else:
                z = coefficients(name, quality)
                tables = [opt.optimal_table(h) for h in j420.symbol_hist(z, restart)]
                scan = j420.scan_from_coefficients(z, restart, tables)
            _REF[key] = (scan, b"".join(opt.table_bytes(t) for t in tables))
        else:
            _REF[key] = (j420.scan(a, quality, restart) if j420.is_gray(a) else j420.scan_from_coefficients(coefficients(name, quality), restart), None)
    return _REF[key]


def shape_of(a):
    return a.shape[0], a.shape[1], 1 if a.ndim == 2 else a.shape[2]


def run_scans(ctx, images, quality, restart, optimal=False, pad=0, caps=None, slot=0, subsampling=capi.JPEG_420):
    """-> [(length, the out buffer's bytes with its guard, the image's table bytes or None)] of ONE gs360_jpeg_scan_sub_u8 call; rows
    padded by `pad` bytes.  The guards behind the lengths and the tables are checked here."""
    bufs, jobs = [], []
    try:
        for k, a in enumerate(images):
            H, W, C = shape_of(a)
            stride = W * C + pad
            rows = np.full((H, stride), 0xEE, np.uint8)
            rows[:, :W * C] = a.reshape(H, W * C)
            src = ctx.to_device(rows)
            cap = jpegenc.scan_bound(H, W, C, restart, "4:2:0" if subsampling == capi.JPEG_420 else "4:4:4") if caps is None else caps[k]
            out = ctx.alloc(cap + GUARD)
            ctx.memset(out, 0xA5, slot)       # asynchronous: on the stream the scan kernels follow on
            bufs += [src, out]
            jobs.append((src, H, W, C, stride if pad else 0, out, cap))
        n = len(jobs)
        d_len = ctx.alloc(8 * n + GUARD)
        d_tab = ctx.alloc(TB * n + GUARD) if optimal else None
        bufs += [d_len] + ([d_tab] if optimal else [])
        ctx.memset(d_len, 0xA5, slot)
        if optimal:
            ctx.memset(d_tab, 0xA5, slot)
        ctx.jpeg_scan_sub_dev(jobs, d_len, d_tab, quality=quality, restart=restart, subsampling=subsampling, slot=slot)
        raw_len = ctx.download(d_len, (8 * n + GUARD,), np.uint8, slot)
        assert np.all(raw_len[8 * n:] == 0xA5)
        raw_tab = None
        if optimal:
            raw_tab = ctx.download(d_tab, (TB * n + GUARD,), np.uint8, slot)
            assert np.all(raw_tab[TB * n:] == 0xA5)
        lengths = raw_len[:8 * n].view(np.uint64)
        return [(int(ln), ctx.download(j[5], (j[6] + GUARD,), np.uint8, slot), raw_tab[k * TB:(k + 1) * TB].tobytes() if optimal else None)
                for k, (ln, j) in enumerate(zip(lengths, jobs))]
    finally:
        for b in bufs:
            ctx.free(b)


def check(name, result, wanted):
    n, data, tables = result
    scan, wtab = wanted
    if wtab is not None:
        assert tables == wtab, (name, [list(tables[t * 272:t * 272 + 16]) for t in range(4)], [list(wtab[t * 272:t * 272 + 16]) for t in range(4)])
    assert n == len(scan), (name, n, len(scan))
    got = data[:n].tobytes()
    if got != scan:
        at = next(i for i in range(n) if got[i] != scan[i])
        raise AssertionError(f"{name}: the scans part at byte {at} of {n}")
    assert np.all(data[-GUARD:] == 0xA5), name


@pytest.mark.parametrize("restart", j420.RESTARTS)
@pytest.mark.parametrize("quality", j420.QUALITIES)
def test_every_shape_in_one_call_matches_the_restatement(ctx, quality, restart):
    got = run_scans(ctx, [IMAGES[n] for n in NAMES], quality, restart)
    for name, res in zip(NAMES, got):
        print(f"{name} q={quality} Ri={restart}: {res[0]} bytes (restatement {len(want(name, quality, restart)[0])})")
        check(name, res, want(name, quality, restart))


@pytest.mark.parametrize("restart", [1, 8])
def test_ladder_and_chroma_extremes(ctx, restart):
    names = ["32x48 ladder", "16x96 blue/yellow", "16x96 red/cyan"]
    got = run_scans(ctx, [IMAGES[n] for n in names], 100, restart)
    for name, res in zip(names, got):
        check(name, res, want(name, 100, restart))


def test_twenty_jobs_split_into_launch_batches(ctx):
    names = [n for n in NAMES if n != "24x520 noise"][:10] * 2       # 20 jobs: the 16-job launch batches split inside the set
    assert len(names) == 20 > capi.MAX_VIEWS
    for optimal in (False, True):
        got = run_scans(ctx, [IMAGES[n] for n in names], 75, 8, optimal=optimal)
        for name, res in zip(names, got):
            check(name, res, want(name, 75, 8, optimal))


def test_padded_rows_give_the_same_scans(ctx):
    names = ["37x53 noise", "75x100 gray", "17x15 smooth", "24x520 noise", "1x1 smooth"]
    for pad in (1, 2, 7):                       # rows that start on every byte alignment
        got = run_scans(ctx, [IMAGES[n] for n in names], 95, 3, pad=pad)
        for name, res in zip(names, got):
            check(name, res, want(name, 95, 3))


def test_a_capacity_one_byte_short_reports_overflow(ctx):
    names = ["37x53 noise", "75x100 photo", "75x100 gray"]
    for optimal in (False, True):
        wants = [want(n, 100, 8, optimal) for n in names]
        caps = [len(wants[0][0]), len(wants[1][0]) - 1, len(wants[2][0]) + 3]      # exact fit, one short, roomy
        got = run_scans(ctx, [IMAGES[n] for n in names], 100, 8, optimal=optimal, caps=caps)
        check(names[0], got[0], wants[0])
        assert got[1][0] == capi.JPEG_OVERFLOW
        assert np.all(got[1][1] == 0xA5)                                   # buffer and guard untouched
        assert got[1][2] == wants[1][1]                                    # optimal: the tables do not depend on the capacity
        check(names[2], got[2], wants[2])


def test_two_calls_give_identical_bytes(ctx):
    a = run_scans(ctx, [IMAGES[n] for n in NAMES], 95, 8, optimal=True)
    b = run_scans(ctx, [IMAGES[n] for n in NAMES], 95, 8, optimal=True)
    for name, ra, rb in zip(NAMES, a, b):
        assert ra[0] == rb[0] and ra[2] == rb[2] and ra[1].tobytes() == rb[1].tobytes(), name


@pytest.mark.parametrize("quality,restart", [(100, 8), (75, 3), (95, 65535), (1, 1)])
def test_optimal_tables_and_scans_match_the_restatement(ctx, quality, restart):
    names = ["37x53 noise", "75x100 photo", "24x520 noise", "75x100 gray", "16x96 red/cyan"]
    got = run_scans(ctx, [IMAGES[n] for n in names], quality, restart, optimal=True)
    for name, res in zip(names, got):
        check(name, res, want(name, quality, restart, True))
        if IMAGES[name].ndim == 2:
            assert res[2][2 * 272:] == bytes(2 * 272), name                # gray: tables 2 and 3 are zero


def test_444_through_the_new_entry_point_is_the_existing_scan(ctx):
    import jpegenc_np as ref
    names = ["37x53 noise", "75x100 gray", "17x15 smooth"]
    got = run_scans(ctx, [IMAGES[n] for n in names], 95, 8, subsampling=capi.JPEG_444)
    for name, res in zip(names, got):
        check(name, res, (ref.scan(IMAGES[name], 95, 8), None))
    got = run_scans(ctx, [IMAGES[n] for n in names], 95, 8, optimal=True, subsampling=capi.JPEG_444)
    for name, res in zip(names, got):
        scan, tables = opt.scan_optimal(IMAGES[name], 95, 8)
        check(name, res, (scan, b"".join(opt.table_bytes(t) for t in tables)))


def test_scan_bound(ctx):
    L = ctx.L
    n, m = ct.c_size_t(0), ct.c_size_t(0)
    for a in IMAGES.values():
        H, W, C = shape_of(a)
        for restart in j420.RESTARTS:
            assert L.gs360_jpeg_scan_bound_sub(H, W, C, restart, capi.JPEG_420, ct.byref(n)) == 0
            mcus = j420.mcus(H, W, C)
            assert n.value == 416 * j420.blocks(H, W, C) + 3 * ((mcus + restart - 1) // restart), (H, W, C, restart)
            assert jpegenc.scan_bound(H, W, C, restart, "4:2:0") == n.value
            assert L.gs360_jpeg_scan_bound(H, W, C, restart, ct.byref(m)) == 0
            if C == 1:
                assert n.value == m.value
            assert L.gs360_jpeg_scan_bound_sub(H, W, C, restart, capi.JPEG_444, ct.byref(n)) == 0 and n.value == m.value
            assert jpegenc.scan_bound(H, W, C, restart) == m.value
    assert L.gs360_jpeg_scan_bound_sub(8, 8, 3, 8, 1, ct.byref(n)) == -1
    assert L.gs360_jpeg_scan_bound_sub(8, 8, 3, 8, capi.JPEG_420, None) == -1
    assert L.gs360_jpeg_scan_bound_sub(8, 8, 4, 8, capi.JPEG_420, ct.byref(n)) == -4


def test_argument_errors(ctx):
    src = ctx.to_device(np.zeros((8, 8, 4), np.uint8))
    out, d_len, d_tab = ctx.alloc(4096), ctx.alloc(8), ctx.alloc(TB)
    try:
        good = (src, 8, 8, 3, 0, out, 4096)
        for sub in (1, 3, -1):
            for tab in (None, d_tab):
                with pytest.raises(gs360.Gs360Error) as e:
                    ctx.jpeg_scan_sub_dev([good], d_len, tab, quality=90, restart=8, subsampling=sub)
                assert e.value.code == -1, sub
        for job, q, ri, code in [((src, 8, 8, 4, 0, out, 4096), 90, 8, -4), ((src, 8, 8, 2, 0, out, 4096), 90, 8, -4),
                                 (good, 0, 8, -1), (good, 101, 8, -1), (good, 90, 0, -1), (good, 90, 65536, -1),
                                 ((src, 0, 8, 3, 0, out, 4096), 90, 8, -1), ((src, 8, 65536, 3, 0, out, 4096), 90, 8, -1),
                                 ((src, 8, 8, 3, 23, out, 4096), 90, 8, -1)]:
            for tab in (None, d_tab):
                with pytest.raises(gs360.Gs360Error) as e:
                    ctx.jpeg_scan_sub_dev([job], d_len, tab, quality=q, restart=ri, subsampling=capi.JPEG_420)
                assert e.value.code == code, (job[1:5], q, ri)
        L = ctx.L
        assert L.gs360_jpeg_scan_sub_u8(ctx.handle, None, 1, 90, 8, capi.JPEG_420, d_len.ptr, None, 0) == -1
        assert L.gs360_jpeg_scan_sub_u8(ctx.handle, None, 0, 90, 8, capi.JPEG_420, None, None, 0) == 0
        assert L.gs360_jpeg_scan_sub_u8(ctx.handle, None, -1, 90, 8, capi.JPEG_420, None, None, 0) == -1
    finally:
        for b in (src, out, d_len, d_tab):
            ctx.free(b)


def test_encode_device_files_equal_the_restatement_and_decode_in_pillow(ctx):
    Image = pytest.importorskip("PIL.Image")
    from PIL import JpegImagePlugin
    names = ["75x100 photo", "75x100 gray", "1x1 smooth", "33x47 smooth", "32x48 ladder"]
    imgs = [IMAGES[n] for n in names]
    std = jpegenc.encode_device(ctx, imgs, quality=95, restart=8, subsampling="4:2:0")
    best = jpegenc.encode_device(ctx, imgs, quality=95, restart=8, huffman="optimal", subsampling="4:2:0")
    for name, a, s, b in zip(names, imgs, std, best):
        assert s == j420.encode(a, 95, 8), name
        assert b == j420.encode_optimal(a, 95, 8), name
        im = Image.open(io.BytesIO(s))
        assert np.asarray(im).shape == a.shape and np.array_equal(np.asarray(im), np.asarray(Image.open(io.BytesIO(b)))), name
        if a.ndim == 3:
            assert JpegImagePlugin.get_sampling(im) == 2, name
    import jpegenc_np as ref
    noise = ref.noise_image(24, 40, 1)
    assert len(j420.scan(noise, 100, 8)) > noise.size               # gray noise at quality 100 needs more than its raw size ...
    d, d2 = ctx.to_device(noise), ctx.to_device(IMAGES["37x53 noise"])
    try:                                        # ... so it is coded again into a buffer of the bound; its neighbour is not
        with ctx.slot_locks[0]:
            f, f2 = jpegenc.encode_buffers(ctx, [(d, 24, 40, 1), (d2, 37, 53, 3)], 100, 8, 0, "optimal", "4:2:0", raw_capacity=True)
        assert f == j420.encode_optimal(noise, 100, 8) and f2 == j420.encode_optimal(IMAGES["37x53 noise"], 100, 8)
    finally:
        ctx.free(d)
        ctx.free(d2)
    with pytest.raises(ValueError):
        jpegenc.encode_device(ctx, [IMAGES["1x1 smooth"]], subsampling="4:2:2")
