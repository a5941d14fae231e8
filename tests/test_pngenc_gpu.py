"""The device PNG encoder (gs360_png_deflate, csrc/gs360_png.hip) against the NumPy restatement of PNG-SPEC v1 (tests/pngenc_np.py): every
deflate stream, length and Adler-32 partial sum through the C ABI, byte for byte, and the size conditions on the device's files."""
import numpy as np
import pytest

from gs360 import capi, pngenc

import pngenc_cases as cases
import pngenc_np as ref
from test_pngenc_cpu import check_size_conditions
from util import CountingPool

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


def check(names, got, want=want):
    """want: name -> (deflate bytes, Adler pairs, ...) (tests/test_pngenc_alphabet_gpu.py brings its own fixtures')"""
    assert len(names) == len(got)
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


_RECODE = {}


def recode_set():
    """-> (images, their whole files, the indices coded again), computed once: a tall one-pixel noise image whose 32 000 filtered bytes
    deflate past its first capacity H * W * C * bps + 4096, small photo-like cases of both depths, and a smooth image far below its"""
    if not _RECODE:
        noise = np.random.default_rng(20261020).integers(0, 256, size=(16000, 1, 1)).astype(np.uint8)
        images = [noise, IMAGES["c3_u8"], IMAGES["c1_u16"], cases._photo(64, 64, 3, np.uint8, 21)]
        files, longer = [], set()
        for i, im in enumerate(images):
            n = len(ref.deflate(im)[0])
            print(f"image {i} {im.shape} {im.dtype}: restated stream {n} bytes, first capacity {im.nbytes + 4096}")
            files.append(ref.encode(im))
            if n > im.nbytes + 4096:
                longer.add(i)
        _RECODE.update(images=images, files=files, longer=longer)
    return _RECODE["images"], _RECODE["files"], _RECODE["longer"]


def test_streams_past_their_first_capacity_are_coded_again_under_pool_allocators(ctx):
    """pngenc.deflate_items as the engine calls it (raw-size first capacities, taking and giving callables over a pool): the files
    equal the restatement's, exactly the items whose restated stream exceeds the first capacity were coded again, and everything taken
    but the returned stream buffers went back."""
    images, wants, longer = recode_set()
    assert 0 < len(longer) < len(images)                 # both branches run
    pool = CountingPool(ctx)
    srcs = [ctx.to_device(im) for im in images]
    items = [(d, im.shape[0], im.shape[1], im.shape[2], im.dtype.itemsize, 0) for d, im in zip(srcs, images)]
    try:
        with ctx.slot_locks[0]:
            streams = pngenc.deflate_items(ctx, items, pool.take, pool.give, 0)
        assert pool.takes == pool.gives + len(streams)
        recoded = {i for i, ((d, _n, _a), im) in enumerate(zip(streams, images)) if d.nbytes != im.nbytes + 4096}
        assert recoded == longer
        for i, ((d, n, adler), (_s, H, W, C, bps, _st)) in enumerate(zip(streams, items)):
            assert d.nbytes == (pngenc.bound(H, W, C, bps) if i in longer else H * W * C * bps + 4096), i
            assert pngenc.assemble(H, W, C, bps, ctx.download(d, (n,), np.uint8).tobytes(), adler) == wants[i], i
        for d, _n, _a in streams:
            pool.give(d)
        assert pool.takes == pool.gives
    finally:
        pool.close()
        for d in srcs:
            ctx.free(d)


def test_the_engine_replaces_the_pinned_block_of_exactly_the_png_views_coded_again(tmp_path):
    """The engine's PNG step itself, without a render: a device state of its own, hand-made view outputs and pinned blocks.  Its views
    share channel count and depth: gray 8-bit, the tall noise image (coded again) and a smooth one (not)."""
    from gs360 import devcodec, engine
    images = [recode_set()[0][0], cases._photo(64, 64, 1, np.uint8, 22)]
    wants = [recode_set()[1][0], ref.encode(images[1])]
    longer = {i for i, im in enumerate(images) if len(ref.deflate(im)[0]) > im.nbytes + 4096}
    assert longer == {0}
    st = engine._DeviceState(0)
    try:
        d_out = [st.ctx.to_device(im) for im in images]
        blocks = [st.ctx.pinned(im.nbytes) for im in images]
        h_out = list(blocks)
        with st.ctx.slot_locks[0]:
            out = engine.Engine._encode_views(None, st, st.ctx, 0, d_out, h_out, [im.shape[:2] for im in images], 1, devcodec.PngMode(), 1)
        for i, view in enumerate(out):
            engine._write_view(tmp_path / f"{i}.png", view, None)
            assert (tmp_path / f"{i}.png").read_bytes() == wants[i], i
            assert (h_out[i] is not blocks[i]) == (i in longer), i
            assert (h_out[i].nbytes > blocks[i].nbytes) == (i in longer), i
        assert st.stats["png_device_images"] == len(images) and st.stats["png_device_bytes"] == sum(len(w) for w in wants)
    finally:
        st.ctx.close()


def test_chunks_past_one_round_of_the_placement_land_at_their_offsets(ctx):
    """257 chunks, one more than the 256 the placement kernel scans per round, of different lengths (4097 x 4095 gray zeros, row y
    opening with (37 * y) % 97 non-zero bytes: identical chunks would hide a misplaced one): length, bytes, guard and all 257 Adler
    pairs of one call."""
    rng = np.random.default_rng(20261021)
    img = np.zeros((4097, 4095, 1), np.uint8)
    for y in range(img.shape[0]):
        img[y, :(37 * y) % 97, 0] = rng.integers(1, 256, (37 * y) % 97)
    assert pngenc.n_chunks(4097, 4095, 1, 1) == 257
    deflated, parts = ref.deflate(img)
    (n, data, sums), = run_deflate(ctx, [img])
    print(f"{n} bytes (restatement {len(deflated)}), {len(sums)} chunks")
    assert n == len(deflated)
    assert data[:n].tobytes() == deflated
    assert (data[n:] == 0xA5).all()
    assert len(sums) == 257 and sums == [p[:2] for p in parts]
