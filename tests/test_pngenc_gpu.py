"""The device PNG encoder (gs360_png_deflate, csrc/gs360_png.hip) against the NumPy restatement of PNG-SPEC v1 (tests/pngenc_np.py): every
deflate stream, length and Adler-32 partial sum through the C ABI, byte for byte, and the size conditions on the device's files."""
import numpy as np
import pytest

from gs360 import capi, pngenc

import pngenc_cases as cases
import pngenc_np as ref
from test_pngenc_cpu import check_size_conditions

pytestmark = pytest.mark.gpu

GUARD = 64
IMAGES = cases.cases()
_REF = {}


def want(name):
    """-> (deflate bytes, [(adler a, adler b)] per chunk, the whole file) of the restatement, computed once"""
    if name not in _REF:
        deflated, parts = ref.deflate(IMAGES[name])
        _REF[name] = (deflated, [p[:2] for p in parts], ref.encode(IMAGES[name]))
    return _REF[name]


def run_deflate(ctx, images, pad=0, offset=0, caps=None, slot=0):
    """-> [(length, the out buffer's bytes with its guard, the job's Adler partials)] of ONE gs360_png_deflate call; rows padded by
    `pad` bytes and the first row `offset` bytes into its buffer"""
    bufs, jobs, counts = [], [], []
    try:
        for k, a in enumerate(images):
            H, W, C = a.shape
            bps = a.dtype.itemsize
            stride = W * C * bps + pad
            rows = np.full((H, stride), 0xEE, np.uint8)
            rows[:, :W * C * bps] = np.ascontiguousarray(a).view(np.uint8).reshape(H, W * C * bps)
            src = ctx.to_device(np.concatenate([np.full(offset, 0xDD, np.uint8), rows.reshape(-1)]))
            cap = pngenc.bound(H, W, C, bps) if caps is None else caps[k]
            out = ctx.alloc(cap + GUARD)
            ctx.memset(out, 0xA5, slot)       # asynchronous: on the stream the encoder's kernels follow on
            bufs += [src, out]
            jobs.append((src.ptr + offset, H, W, C, bps, stride if pad else 0, out, cap))
            counts.append(pngenc.n_chunks(H, W, C, bps))
        d_len, d_adler = ctx.alloc(8 * len(jobs)), ctx.alloc(8 * sum(counts))
        bufs += [d_len, d_adler]
        ctx.png_deflate_dev(jobs, d_len, d_adler, slot)
        lengths = ctx.download(d_len, (len(jobs),), np.uint64, slot)
        sums = ctx.download(d_adler, (sum(counts), 2), np.uint32, slot)
        at = np.concatenate([[0], np.cumsum(counts)])
        return [(int(n), ctx.download(j[6], (j[7] + GUARD,), np.uint8, slot), [tuple(int(v) for v in r) for r in sums[at[k]:at[k + 1]]])
                for k, (n, j) in enumerate(zip(lengths, jobs))]
    finally:
        for b in bufs:
            ctx.free(b)


def check(names, got):
    for name, (n, data, sums) in zip(names, got):
        deflated, parts, _png = want(name)
        print(f"{name}: {n} bytes (restatement {len(deflated)})")
        assert n == len(deflated), name
        assert data[:n].tobytes() == deflated, name
        assert (data[n:] == 0xA5).all(), name            # nothing behind the stream
        assert sums == parts, name


def test_every_case_in_one_call_matches_the_restatement(ctx):
    """a batch of more than GS360_MAX_VIEWS images of different sizes, channels and depths"""
    names = list(IMAGES)
    assert len(names) > capi.MAX_VIEWS
    check(names, run_deflate(ctx, [IMAGES[n] for n in names]))


@pytest.mark.parametrize("name", ["deg_1x1", "deg_300x1", "runs", "fibonacci", "chunk_over1"])
def test_a_case_alone_matches_the_restatement(ctx, name):
    check([name], run_deflate(ctx, [IMAGES[name]]))


def test_padded_rows_and_an_offset_base_pointer(ctx):
    names = [f"c{C}_{tag}" for C in (1, 3, 4) for tag in ("u8", "u16")] + ["seams_coprime"]
    check(names, run_deflate(ctx, [IMAGES[n] for n in names], pad=10, offset=6))


def test_a_capacity_that_is_too_small_is_reported_and_nothing_is_written(ctx):
    names = ["c3_u8", "noise", "c1_u16"]
    sizes = [len(want(n)[0]) for n in names]
    caps = [pngenc.bound(37, 53, 3, 1), sizes[1] - 1, sizes[2]]                    # the second one byte short, the third exact
    got = run_deflate(ctx, [IMAGES[n] for n in names], caps=caps)
    assert got[1][0] == capi.PNG_OVERFLOW and (got[1][1] == 0xA5).all()
    check([names[0], names[2]], [got[0], got[2]])


def test_argument_errors(ctx):
    src, out, d_len, d_adler = ctx.alloc(64), ctx.alloc(4096), ctx.alloc(8), ctx.alloc(8)
    try:
        for job in ((src, 0, 4, 3, 1, 0, out, 4096), (src, 4, 4, 2, 1, 0, out, 4096), (src, 4, 4, 3, 3, 0, out, 4096),
                    (src, 4, 4, 3, 1, 11, out, 4096), (src.ptr + 1, 2, 2, 1, 2, 0, out, 4096)):
            with pytest.raises(capi.Gs360Error):
                ctx.png_deflate_dev([job], d_len, d_adler)
    finally:
        for b in (src, out, d_len, d_adler):
            ctx.free(b)


def test_encode_device_writes_the_restatements_files(ctx):
    names = ["c3_u8", "c4_u16", "chunk_over2", "zeros"]
    files = pngenc.encode_device(ctx, [IMAGES[n] for n in names])
    for name, data in zip(names, files):
        assert data == want(name)[2], name


def test_size_conditions_on_the_device(ctx, tmp_path):
    check_size_conditions(lambda img: pngenc.encode_device(ctx, [img])[0], tmp_path)
