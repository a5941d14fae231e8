"""The device mask-finishing chain (gs360_mask_finish_u8, csrc/gs360_maskmorph.hip) against the NumPy restatement of MSK-SPEC v1
(tests/maskfinish_np.py): every output byte and every count through the C ABI, with no tolerance."""
import dataclasses

import numpy as np
import pytest

from gs360 import capi, maskfinish

import maskfinish_cases as cases
import maskfinish_np as ref

pytestmark = pytest.mark.gpu

GUARD = 64
CASES = cases.cases()
LIMITS = cases.limit_cases()                             # run by tests/test_mask_limits_gpu.py alone: no test here names one
CHANNELS = {"mask": 1, "rgba": 4, "keep": 3, "remove": 3}
_REF = {}


def case_of(name):
    return CASES[name] if name in CASES else LIMITS[name]


def want(name, kind="mask", invert=True, params=None, use_add=True):
    """-> (the restatement's output, its count), computed once per variant"""
    key = (name, kind, invert, params and dataclasses.astuple(params), use_add)
    if key not in _REF:
        c = case_of(name)
        shape = cases.shape_of(c)
        _REF[key] = ref.finish(c.raw, params or c.params, c.add if use_add else None, cases.image_for(shape) if kind != "mask" else None,
                               kind, invert, shape)
    return _REF[key]


def padded(ctx, a, pad, offset, bufs):
    """rows of `a` (H x row bytes) `pad` bytes apart beyond their length, the first `offset` bytes into the buffer -> (address, stride)"""
    a = np.ascontiguousarray(a).reshape(a.shape[0], -1)
    rows = np.full((a.shape[0], a.shape[1] + pad), 0xEE, np.uint8)
    rows[:, :a.shape[1]] = a
    bufs.append(ctx.to_device(np.concatenate([np.full(offset, 0xDD, np.uint8), rows.reshape(-1)])))
    return bufs[-1].ptr + offset, a.shape[1] + pad if pad else 0


def run_finish(ctx, names, kind="mask", invert=True, pad=0, offset=0, params=None, use_add=True, slot=0):
    """-> [(output array, count)] of ONE gs360_mask_finish_u8 call on the named fixtures; checks the guards behind every output and
    behind the scratch"""
    C = CHANNELS[kind]
    shapes = [cases.shape_of(case_of(n)) for n in names]
    bufs, jobs, outs = [], [], []
    try:
        for n, (H, W) in zip(names, shapes):
            c = case_of(n)
            (j,), keep = maskfinish.build_jobs([(H, W)], params or c.params, kind, invert)
            bufs.append(keep)                             # (the element rows stay alive until the call has read them)
            if c.raw is not None:
                j.src, j.src_stride = padded(ctx, c.raw, pad, offset, bufs)
            if c.add is not None and use_add:
                j.add, j.add_stride = padded(ctx, c.add, pad, offset, bufs)
            if kind != "mask":
                j.image, j.image_stride = padded(ctx, cases.image_for((H, W)), pad, offset, bufs)
            stride = W * C + pad
            out = ctx.alloc(offset + H * stride + GUARD)
            ctx.memset(out, 0xA5, slot)
            outs.append(out)
            j.dst, j.dst_stride = out.ptr + offset, stride if pad else 0
            jobs.append(j)
        need = ctx.mask_finish_scratch(jobs)
        scratch, counts = ctx.alloc(need + GUARD), ctx.alloc(4 * len(jobs))
        outs += [scratch, counts]
        ctx.memset(scratch, 0xA5, slot)
        ctx.mask_finish_dev(jobs, scratch, counts, slot, scratch_bytes=need)
        got_counts = ctx.download(counts, (len(jobs),), np.uint32, slot)
        assert (ctx.download(scratch, (need + GUARD,), np.uint8, slot)[need:] == 0xA5).all(), "scratch guard"
        res = []
        for n, (H, W), out, cnt in zip(names, shapes, outs, got_counts):
            stride = W * C + pad
            raw = ctx.download(out, (offset + H * stride + GUARD,), np.uint8, slot)
            assert (raw[:offset] == 0xA5).all() and (raw[offset + H * stride:] == 0xA5).all(), (n, "output guard")
            rows = raw[offset:offset + H * stride].reshape(H, stride)
            assert (rows[:, W * C:] == 0xA5).all(), (n, "row padding")
            res.append((rows[:, :W * C].reshape((H, W) if C == 1 else (H, W, C)).copy(), int(cnt)))
        return res
    finally:
        for b in bufs + outs:
            if isinstance(b, capi.DeviceBuffer):
                ctx.free(b)


def check(names, got, **variant):
    for name, (out, count) in zip(names, got):
        exp, n = want(name, **variant)
        print(f"{name}: {count} set (restatement {n}), {int((out != exp).sum())} bytes differ")
        assert count == n, name
        assert np.array_equal(out, exp), name


def test_every_fixture_in_one_call_matches_the_restatement(ctx):
    """a batch of more than GS360_MAX_VIEWS masks of mixed sizes, elements and strips"""
    names = list(CASES)
    assert len(names) > capi.MAX_VIEWS
    check(names, run_finish(ctx, names))


@pytest.mark.parametrize("name", ["1x1-set", "1x70-corners", "70x1-corners", "40x33-", "33x64-noise", "big-crowd-p77", "none-add-only"])
def test_a_fixture_alone_matches_the_restatement(ctx, name):
    full = next(n for n in CASES if n.startswith(name))
    check([full], run_finish(ctx, [full]))


STEP_NAMES = [n for n in CASES if n.startswith(("37x97-", "26x65-", "5x31-", "big-blobs"))]
STEPS = {"close": maskfinish.Params(close=6, expand_pixels=0, edge_fuse_pixels=0),
         "close5": maskfinish.Params(close=5, expand_pixels=0, edge_fuse_pixels=0),
         "expand": maskfinish.Params(close=1, expand_pixels=15, edge_fuse_pixels=0),
         "expand-wide": maskfinish.Params(close=1, expand_pixels=40, edge_fuse_pixels=0),
         "fuse": maskfinish.Params(close=1, expand_pixels=0, edge_fuse_pixels=5),
         "add": maskfinish.Params(close=1, expand_pixels=0, edge_fuse_pixels=0)}


@pytest.mark.parametrize("step", list(STEPS))
def test_each_step_alone(ctx, step):
    """one step of the chain per call, so that a failure names its kernel: morph (close, expand), fuse, finish (add)"""
    use_add = step == "add"
    check(STEP_NAMES, run_finish(ctx, STEP_NAMES, params=STEPS[step], use_add=use_add), params=STEPS[step], use_add=use_add)


def test_thresholded_pack_alone(ctx):
    p = maskfinish.Params(close=1, expand_pixels=0, edge_fuse_pixels=0, thresh=200)     # the corners fixtures hold 200 and 255
    names = [n for n in CASES if "-corners-" in n]
    check(names, run_finish(ctx, names, params=p, use_add=False), params=p, use_add=False)


@pytest.mark.parametrize("kind", ["mask", "rgba"])
def test_padded_rows_and_an_offset_base_pointer(ctx, kind):
    names = [n for n in CASES if n.startswith(("9x63-", "40x33-", "12x13-"))] + ["none-add-only"]
    check(names, run_finish(ctx, names, kind=kind, pad=11, offset=7), kind=kind)


@pytest.mark.parametrize("invert", [True, False])
@pytest.mark.parametrize("kind", ["mask", "rgba", "keep", "remove"])
def test_the_output_kinds_both_polarities_and_the_empty_mask_branches(ctx, kind, invert):
    names = [next(n for n in CASES if n.startswith(p)) for p in ("40x33-disc", "17x32-clear", "37x97-blobs")] + ["none-empty", "none-add-only"]
    got = run_finish(ctx, names, kind=kind, invert=invert)
    assert got[3][1] == 0 and got[0][1] > 0              # an empty mask among them
    check(names, got, kind=kind, invert=invert)


def test_limits_are_unsupported_and_write_nothing(ctx):
    src, out, scratch, counts = ctx.alloc(64), ctx.alloc(4096), ctx.alloc(4096), ctx.alloc(4)
    try:
        for b in (out, scratch, counts):
            ctx.memset(b, 0xA5)
        for shape, params in (((8, 8), maskfinish.Params(expand_pixels=513, edge_fuse_pixels=0)),
                              ((1, 32769), maskfinish.Params(edge_fuse_pixels=0)), ((32769, 1), maskfinish.Params(edge_fuse_pixels=0)),
                              ((1100, 1030), maskfinish.Params(edge_fuse_pixels=capi.MASK_MAX_FUSE + 1))):
            (j,), _keep = maskfinish.build_jobs([shape], params)
            j.src, j.dst = src.ptr, out.ptr
            with pytest.raises(capi.Gs360Error) as e:
                ctx.mask_finish_scratch([j])
            assert e.value.code == -4
            with pytest.raises(capi.Gs360Error) as e:
                ctx.mask_finish_dev([j], scratch, counts)
            assert e.value.code == -4
        (j,), _keep = maskfinish.build_jobs([(8, 8)], maskfinish.Params(expand_pixels=512, edge_fuse_pixels=0))
        j.src, j.dst = src.ptr, out.ptr
        assert ctx.mask_finish_scratch([j]) > 0                                   # p = 512 is inside
        for b in (out, scratch, counts):
            assert (ctx.download(b, (b.nbytes,), np.uint8) == 0xA5).all()
    finally:
        for b in (src, out, scratch, counts):
            ctx.free(b)


def test_argument_errors(ctx):
    src, out, scratch, counts = ctx.alloc(64), ctx.alloc(4096), ctx.alloc(1 << 16), ctx.alloc(4)
    try:
        def job(**kw):
            (j,), keep = maskfinish.build_jobs([(8, 8)], maskfinish.Params(edge_fuse_pixels=3), kw.pop("kind", "mask"))
            j.src, j.dst = src.ptr, out.ptr
            for k, v in kw.items():
                setattr(j, k, v)
            return j, keep
        for kw in ({"dst": None}, {"kind": "rgba"}, {"src_stride": 7}, {"dst_stride": 7}, {"fuse": 9}, {"thresh": 256}, {"close_rows": None},
                   {"H": 0}):
            j, _keep = job(**kw)
            with pytest.raises(capi.Gs360Error) as e:
                ctx.mask_finish_dev([j], scratch, counts)
            assert e.value.code == -1, kw
        j, _keep = job()
        with pytest.raises(capi.Gs360Error):
            ctx.mask_finish_dev([j], scratch, counts, scratch_bytes=ctx.mask_finish_scratch([j]) - 1)
        bad = np.array([[0, 6]] * 5, np.int32)                                    # a span past the element's 5 columns
        j, _keep = job(close_rows=bad.ctypes.data)
        with pytest.raises(capi.Gs360Error):
            ctx.mask_finish_dev([j], scratch, counts)
    finally:
        for b in (src, out, scratch, counts):
            ctx.free(b)


def test_two_calls_give_identical_bytes(ctx):
    names = [n for n in CASES if n.startswith(("37x97-", "big-blobs"))]
    a, b = run_finish(ctx, names, kind="rgba"), run_finish(ctx, names, kind="rgba", slot=1)
    for (x, nx), (y, ny) in zip(a, b):
        assert nx == ny and x.tobytes() == y.tobytes()


def test_the_public_finish_call(ctx):
    names = [n for n in CASES if n.startswith("40x33-")]
    p = maskfinish.Params(close=5, expand_pixels=3, edge_fuse_pixels=4, thresh=127)
    masks = [CASES[n].raw for n in names] + [(12, 50)]
    adds = [CASES[n].add for n in names] + [None]
    images = [cases.image_for(cases.shape_of(CASES[n])) for n in names] + [cases.image_for((12, 50))]
    outs, counts = maskfinish.finish(ctx, masks, p, adds, images, kind="keep", invert=True)
    for m, a, im, out, n in zip(masks, adds, images, outs, counts):
        exp, cnt = ref.finish(None if isinstance(m, tuple) else m, p, a, im, "keep", True, im.shape[:2])
        assert int(n) == cnt and np.array_equal(out, exp)
    with pytest.raises(ValueError):
        maskfinish.finish(ctx, [np.zeros((10, 10), np.uint8)], maskfinish.Params(edge_fuse_pixels=11))
