"""The device shadow estimate (gs360_mask_shadow_candidates_u8 / gs360_mask_shadow_merge_u8, csrc/gs360_maskshadow.hip) against the
NumPy restatement of MSK-SHADOW v1 (tests/maskshadow_np.py): every stage the calls leave in their scratch (P, C0, C1, C2, clean),
every byte of M and both counts through the C ABI, with no tolerance.  A failure names its stage, and with it its kernel: C0 is the
pixel and the two blur kernels, C1 the plane logic, C2 the morphology, clean the labelling, the areas and the selection."""
import numpy as np
import pytest

from gs360 import capi, maskfinish

import maskshadow_cases as cases
import maskshadow_np as ref

pytestmark = pytest.mark.gpu

GUARD = 64
STAGES = ("P", "C0", "C1", "C2", "clean")
BLUR = cases.blur_cases()
_REF = {}


def want(name, job):
    """the restatement's stages of a job, computed once"""
    if name not in _REF:
        _REF[name] = ref.run_job(job)
    return _REF[name]


def padded(ctx, a, pad, offset, bufs):
    """rows of `a` (H x row bytes) `pad` bytes apart beyond their length, the first `offset` bytes into the buffer -> (address, stride)"""
    a = np.ascontiguousarray(a).reshape(a.shape[0], -1)
    rows = np.full((a.shape[0], a.shape[1] + pad), 0xEE, np.uint8)
    rows[:, :a.shape[1]] = a
    bufs.append(ctx.to_device(np.concatenate([np.full(offset, 0xDD, np.uint8), rows.reshape(-1)])))
    return bufs[-1].ptr + offset, a.shape[1] + pad if pad else 0


def rows_array(rows):
    return np.ascontiguousarray(rows, dtype=np.int32)


def unpack(plane_bytes, H, W):
    pw = (W + 31) // 32
    words = np.frombuffer(plane_bytes[:H * pw * 4].tobytes(), np.uint32).reshape(H, pw)
    bits = (words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
    assert not bits.reshape(H, -1)[:, W:].any(), "bits beyond the image's columns"
    return bits.reshape(H, -1)[:, :W].astype(bool)


def run_shadow(ctx, named_jobs, pad=0, offset=0, slot=0):
    """-> [dict of the stages, M, count_p, count] of ONE candidates call and ONE merge call on the jobs; checks the guards behind
    every output and behind the scratch"""
    bufs, keep, jobs, outs = [], [], [], []
    sdiv = maskfinish.sat_div_table()
    try:
        for _name, c in named_jobs:
            H, W = c.raw.shape
            j = capi.ShadowJob()
            j.H, j.W, j.thresh = H, W, c.thresh
            half = np.ascontiguousarray(c.half, dtype=np.float32)
            keep += [half]
            j.radius, j.weights, j.sdiv = len(half) - 1, half.ctypes.data, sdiv.ctypes.data
            j.t, j.delta_min, j.sat_max, j.min_area = c.t, c.delta_min, c.sat_max, c.min_area
            if c.close > 1:
                keep.append(rows_array(maskfinish.structuring_rows(c.close, c.close)[0]))
                j.close_kw = j.close_kh = c.close
                j.close_rows = keep[-1].ctypes.data
            j.src, j.src_stride = padded(ctx, c.raw, pad, offset, bufs)
            j.image, j.image_stride = padded(ctx, c.img, pad, offset, bufs)
            stride = W + pad
            out = ctx.alloc(offset + H * stride + GUARD)
            ctx.memset(out, 0xA5, slot)
            outs.append(out)
            j.dst, j.dst_stride = out.ptr + offset, stride if pad else 0
            jobs.append(j)
        need = ctx.mask_shadow_scratch(jobs)
        areas = [ctx.mask_shadow_scratch([j]) - 256 for j in jobs]
        assert need == 256 + sum(areas)
        scratch, counts = ctx.alloc(need + GUARD), ctx.alloc(4 * len(jobs))
        outs += [scratch, counts]
        ctx.memset(scratch, 0xA5, slot)
        ctx.mask_shadow_candidates_dev(jobs, scratch, counts, slot, scratch_bytes=need)
        count_p = ctx.download(counts, (len(jobs),), np.uint32, slot)
        for j, (_name, c), n in zip(jobs, named_jobs, count_p):
            for field, (rows, kw, kh) in zip(("near", "sclose", "open"), ref.elements_of(c, int(n))):
                keep.append(rows_array(rows))
                setattr(j, field + "_kw", kw)
                setattr(j, field + "_kh", kh)
                setattr(j, field + "_rows", keep[-1].ctypes.data)
        ctx.mask_shadow_merge_dev(jobs, scratch, counts, slot, scratch_bytes=need)
        count_m = ctx.download(counts, (len(jobs),), np.uint32, slot)
        raw = ctx.download(scratch, (need + GUARD,), np.uint8, slot)
        assert (raw[need:] == 0xA5).all(), "scratch guard"
        res, at = [], 256
        for (name, c), out, area, np_, nm in zip(named_jobs, outs, areas, count_p, count_m):
            H, W = c.raw.shape
            plane = (H * ((W + 31) // 32) * 4 + 255) // 256 * 256
            got = {s: unpack(raw[at + k * plane:at + (k + 1) * plane], H, W) for k, s in enumerate(STAGES)}
            at += area
            stride = W + pad
            m = ctx.download(out, (offset + H * stride + GUARD,), np.uint8, slot)
            assert (m[:offset] == 0xA5).all() and (m[offset + H * stride:] == 0xA5).all(), (name, "output guard")
            rows = m[offset:offset + H * stride].reshape(H, stride)
            assert (rows[:, W:] == 0xA5).all(), (name, "row padding")
            got.update(M=rows[:, :W].copy(), count_p=int(np_), count=int(nm))
            res.append(got)
        return res
    finally:
        for b in bufs + outs:
            ctx.free(b)


def check(named_jobs, got):
    for (name, job), g in zip(named_jobs, got):
        w = want(name, job)
        diff = {s: int((g[s] != w[s]).sum()) for s in STAGES}
        diff["M"] = int((g["M"] != np.where(w["M"], 255, 0)).sum())
        print(f"{name}: person {g['count_p']} (restatement {w['count_p']}), M {g['count']} ({w['count']}), pixels that differ: {diff}")
        for s in STAGES + ("M",):
            assert diff[s] == 0, (name, s)
        assert (g["count_p"], g["count"]) == (w["count_p"], w["count"]), name


@pytest.mark.parametrize("name", list(BLUR))
def test_blur_and_candidates(ctx, name):
    """sides of 1 and below the radius (repeated reflection), both sides below 2 r + 1, and 200 x 333 past every tile edge with a
    padded row pitch and an offset base pointer; the -sign variants turn on the last bit of the blurred value"""
    jobs = [(name, cases.blur_job(BLUR[name]))]
    big = name.startswith("200x333")
    check(jobs, run_shadow(ctx, jobs, pad=13 if big else 0, offset=5 if big else 0))


def label_jobs(H, W):
    return [(f"{H}x{W}-{n}", cases.label_job(n, X)) for n, X in cases.label_planes(H, W).items()]


def test_more_than_one_launch_of_mixed_jobs_in_one_call(ctx):
    """every 97 x 130 labelling fixture and every blur fixture of a small size in one pair of calls: more than GS360_MAX_VIEWS jobs"""
    jobs = label_jobs(*cases.LABEL_SIZES[0]) + [(n, cases.blur_job(c)) for n, c in BLUR.items() if not n.startswith("200x333")]
    assert len(jobs) > capi.MAX_VIEWS
    check(jobs, run_shadow(ctx, jobs))


@pytest.mark.parametrize("name", cases.LABEL_NAMES)
def test_labelling_past_one_tile(ctx, name):
    H, W = cases.LABEL_SIZES[1]
    jobs = [(f"{H}x{W}-{name}", cases.label_job(name, cases.label_planes(H, W)[name]))]
    check(jobs, run_shadow(ctx, jobs, slot=1))


PHOTOS = [("photo-200x333", (200, 333, 11, True)), ("photo-97x130", (97, 130, 12, True)), ("photo-64x80-nobody", (64, 80, 13, False))]


def test_the_whole_chain_stage_by_stage(ctx):
    jobs = [(n, cases.photo_job(*a)) for n, a in PHOTOS]
    got = run_shadow(ctx, jobs)
    check(jobs, got)
    assert got[2]["count"] == 0 and not got[2]["M"].any() and got[0]["clean"].any()


@pytest.mark.parametrize("kind", ["mask", "rgba"])
def test_finish_with_shadow_equals_the_restatements_chain(ctx, kind):
    """M goes on into MSK-SPEC steps 2-6 on the device: the public call against maskfinish_np.finish on the restatement's M"""
    photos = [cases.photograph(*a) for _n, a in PHOTOS]
    images, masks = [p[0] for p in photos], [p[1] for p in photos]
    masks[2] = masks[2].shape                             # no detection, given as a shape
    outs, counts = maskfinish.finish_with_shadow(ctx, masks, cases.CHAIN_PARAMS, cases.CHAIN_SHADOW, None, images, kind=kind)
    for (name, _a), img, raw, out, n in zip(PHOTOS, images, photos, outs, counts):
        exp, cnt = ref.finish_with_shadow(img, raw[1], cases.CHAIN_PARAMS, cases.CHAIN_SHADOW, None, kind, True)
        print(f"{name} {kind}: {int(n)} set (restatement {cnt}), {int((out != exp).sum())} bytes differ")
        assert int(n) == cnt and np.array_equal(out, exp), name
    assert counts[0] > 0 and counts[2] == 0


def test_limits_and_argument_errors_on_the_argument_path(ctx):
    """no plane of such a size is allocated: the jobs are refused before anything is read"""
    src, counts = ctx.alloc(4096), ctx.alloc(4)
    half, sdiv = np.ones(1, np.float32), maskfinish.sat_div_table()

    def job(H=8, W=8, radius=0, **kw):
        j = capi.ShadowJob()
        j.H, j.W, j.radius, j.weights, j.sdiv = H, W, radius, half.ctypes.data, sdiv.ctypes.data
        j.image = j.src = j.dst = src.ptr
        for k, v in kw.items():
            setattr(j, k, v)
        return j
    try:
        for j in (job(32768, 32769), job(32769, 32768), job(40000, 40000), job(radius=256)):      # above 2^30 pixels; radius
            assert j.H * j.W > capi.SHADOW_MAX_PIXELS or j.radius > capi.SHADOW_MAX_RADIUS
            with pytest.raises(capi.Gs360Error) as e:
                ctx.mask_shadow_scratch([j])
            assert e.value.code == -4
            for call in (ctx.mask_shadow_candidates_dev, ctx.mask_shadow_merge_dev):
                with pytest.raises(capi.Gs360Error) as e:
                    call([j], src, counts)
                assert e.value.code == -4
        assert ctx.mask_shadow_scratch([job(radius=255)]) > 0 and ctx.mask_shadow_scratch([job(32768, 32768)]) > 2 ** 33
        for j in (job(H=0), job(radius=-1), job(image=None), job(weights=None), job(image_stride=7), job(thresh=256)):
            with pytest.raises(capi.Gs360Error) as e:
                ctx.mask_shadow_candidates_dev([j], src, counts)
            assert e.value.code == -1
        with pytest.raises(capi.Gs360Error) as e:        # the merge needs its elements
            ctx.mask_shadow_merge_dev([job()], src, counts)
        assert e.value.code == -1
        with pytest.raises(capi.Gs360Error) as e:        # a scratch that is too small
            ctx.mask_shadow_candidates_dev([job(64, 64)], src, counts)
        assert e.value.code == -1
    finally:
        ctx.free(src)
        ctx.free(counts)
