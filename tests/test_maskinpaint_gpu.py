"""The device inpaint stage (gs360_mask_inpaint_u8, csrc/gs360_maskinpaint.hip) against the NumPy restatement of MSK-INPAINT v1
(tests/maskinpaint_np.py) through the C ABI: every byte of the filled image and every `levels` value, with no tolerance; the guards
behind every image, the row padding and the scratch stay untouched."""
import numpy as np
import pytest

from gs360 import capi, maskfinish

import maskfinish_np
import maskinpaint_np as ref
import maskshadow_cases
import maskshadow_np

pytestmark = pytest.mark.gpu

GUARD = 64
_REF = {}


def want(name, img, F, radius=5):
    """the restatement's image and K of a case, computed once"""
    if name not in _REF:
        _REF[name] = ref.inpaint(img, F, radius)
    return _REF[name]


def padded(ctx, a, pad, offset, bufs, slot=0):
    """rows of `a` `pad` bytes apart beyond their length, the first `offset` bytes into a buffer that ends in a guard ->
    (address, stride argument, buffer, row bytes)"""
    a = np.ascontiguousarray(a).reshape(a.shape[0], -1)
    rows = np.full((a.shape[0], a.shape[1] + pad), 0xEE, np.uint8)
    rows[:, :a.shape[1]] = a
    flat = np.concatenate([np.full(offset, 0xDD, np.uint8), rows.reshape(-1), np.full(GUARD, 0xA5, np.uint8)])
    bufs.append(ctx.to_device(flat, slot))
    return bufs[-1].ptr + offset, a.shape[1] + pad if pad else 0, bufs[-1], a.shape[1]


def run_inpaint(ctx, cases, pad=0, offset=0, slot=0):
    """cases: [(img, F, radius)] -> ([filled image], levels) of ONE call; checks every guard"""
    bufs, jobs, images = [], [], []
    try:
        for img, F, radius in cases:
            H, W = F.shape
            j = capi.InpaintJob()
            j.H, j.W, j.radius = H, W, radius
            j.image, j.image_stride, buf, row = padded(ctx, img, pad, offset, bufs, slot)
            images.append((buf, row))
            j.fill, j.fill_stride, _buf, _row = padded(ctx, np.where(F, 200, 0).astype(np.uint8), pad, offset, bufs, slot)
            jobs.append(j)
        need = ctx.mask_inpaint_scratch(jobs)
        scratch, levels = ctx.alloc(need + GUARD), ctx.alloc(4 * len(jobs))
        bufs += [scratch, levels]
        ctx.memset(scratch, 0xA5, slot)
        ctx.mask_inpaint_dev(jobs, scratch, levels, slot, scratch_bytes=need)
        K = ctx.download(levels, (len(jobs),), np.uint32, slot)
        assert (ctx.download(scratch, (need + GUARD,), np.uint8, slot)[need:] == 0xA5).all(), "scratch guard"
        outs = []
        for (img, F, _r), (buf, row) in zip(cases, images):
            H, W = F.shape
            flat = ctx.download(buf, (offset + H * (row + pad) + GUARD,), np.uint8, slot)
            assert (flat[:offset] == 0xDD).all() and (flat[offset + H * (row + pad):] == 0xA5).all(), "image guard"
            rows = flat[offset:offset + H * (row + pad)].reshape(H, row + pad)
            assert (rows[:, row:] == 0xEE).all(), "row padding"
            outs.append(rows[:, :row].reshape(H, W, 3).copy())
        return outs, K
    finally:
        for b in bufs:
            ctx.free(b)


def check(ctx, named, pad=0, offset=0, slot=0):
    """named: [(name, img, F, radius)]: one call, every byte and every K"""
    outs, K = run_inpaint(ctx, [c[1:] for c in named], pad, offset, slot)
    for (name, img, F, radius), out, k in zip(named, outs, K):
        exp, Kw = want(name, img, F, radius)
        wrong = int((out != exp).any(axis=2).sum())
        print(f"{name}: {int(F.sum())} pixels of F, K {int(k)} (restatement {Kw}), {wrong} pixels differ")
        assert int(k) == Kw and wrong == 0, name
        assert np.array_equal(out[~F], img[~F]), (name, "a pixel outside F was written")
    return outs, K


def case(name, H, W, F, seed=1, radius=5):
    return (name, ref.photograph(H, W, seed), F, radius)


def lone_pixel():
    F = np.ones((9, 9), bool)
    F[3, 5] = False
    return case("9x9-lone", 9, 9, F, 4)


def borders():
    F = np.ones((30, 37), bool)
    F[12:15, 17:21] = False
    return case("30x37-borders", 30, 37, F, 5)


CASES = {
    "fixture": lambda: case("fixture", 40, 48, ref.fixture_mask(), 5),
    "fixture-ramp": lambda: ("fixture-ramp", ref.ramp(40, 48, 2, 3, 7), ref.fixture_mask(), 5),
    "width-1": lambda: case("70x1", 70, 1, np.random.default_rng(3).random((70, 1)) < 0.8, 3),
    "height-1": lambda: case("1x70", 1, 70, np.random.default_rng(3).random((1, 70)) < 0.8, 2),
    "a-single-pixel-outside": lone_pixel,
    "deeper-than-two-radii": lambda: case("60x64-deep", 60, 64, ref.discs(60, 64, [(30, 31)], 14), 6),
    "all-four-borders": borders,
    "two-regions": lambda: case("50x300-two", 50, 300, ref.discs(50, 300, [(20, 30), (28, 270)], 9), 7),
    "radius-3": lambda: case("fixture-r3", 40, 48, ref.fixture_mask(), 8, radius=3),
    "radius-8": lambda: case("fixture-r8", 40, 48, ref.fixture_mask(), 8, radius=8),
}


@pytest.mark.parametrize("name", list(CASES))
def test_one_image(ctx, name):
    """the spec's fixture (a photograph and a ramp), sides of one, a single pixel outside F, a region deeper than two radii (K = 15),
    F on all four borders, two regions in a row longer than one workgroup, the smallest and the largest radius"""
    c = CASES[name]()
    _outs, K = check(ctx, [c])
    if name == "deeper-than-two-radii":
        assert K[0] > 10


def test_a_padded_pitch_and_an_offset_base(ctx):
    F = ref.discs(53, 75, [(20, 20), (52, 74), (0, 40)], 8)
    check(ctx, [case("53x75-padded", 53, 75, F, 9)], pad=13, offset=5, slot=1)


def test_noise_clamps_at_both_ends(ctx):
    F = ref.fixture_mask()
    noise = np.random.default_rng(9).choice(np.array([0, 255], np.uint8), size=F.shape + (3,))
    outs, _K = check(ctx, [("noise", noise, F, 5)])
    assert (outs[0][F] == 0).any() and (outs[0][F] == 255).any()


def test_empty_and_full_masks_leave_the_image_alone(ctx):
    img = ref.photograph(12, 9, 1)
    outs, K = check(ctx, [("empty", img, np.zeros((12, 9), bool), 5), ("full", img, np.ones((12, 9), bool), 5)])
    assert list(K) == [0, 0] and np.array_equal(outs[0], img) and np.array_equal(outs[1], img)


def test_a_batch_of_three_sizes_one_of_them_empty(ctx):
    named = [CASES["fixture"](), ("empty-20x33", ref.photograph(20, 33, 2), np.zeros((20, 33), bool), 5), CASES["deeper-than-two-radii"]()]
    _outs, K = check(ctx, named)
    assert K[1] == 0 and len(set(int(k) for k in K)) == 3


def test_more_jobs_than_one_launch_holds(ctx):
    named = []
    for k in range(capi.MAX_VIEWS + 3):
        H, W = 14 + k, 31 - k
        named.append(case(f"many-{k}", H, W, ref.discs(H, W, [(H // 2, W // 2)], 3 + k % 4), 20 + k))
    check(ctx, named)


def test_two_runs_give_the_same_bytes(ctx):
    c = CASES["two-regions"]()
    a, Ka = run_inpaint(ctx, [c[1:]])
    b, Kb = run_inpaint(ctx, [c[1:]], slot=1)
    assert np.array_equal(a[0], b[0]) and list(Ka) == list(Kb)


def test_k_of_4095_runs_and_4096_is_refused(ctx):
    """a row whose only pixel outside F is its first: K = W - 1.  4095 launches of one pixel each; one level more is refused and the
    image stays as it was"""
    F = np.ones((1, 4096), bool)
    F[0, 0] = False
    img = ref.photograph(1, 4096, 3)
    _outs, K = check(ctx, [("1x4096", img, F, 5)])
    assert K[0] == capi.INPAINT_MAX_LEVEL
    F = np.ones((1, 4097), bool)
    F[0, 0] = False
    img = ref.photograph(1, 4097, 3)
    with pytest.raises(ValueError):
        ref.inpaint(img, F)
    with pytest.raises(capi.Gs360Error) as e:
        run_inpaint(ctx, [(img, F, 5)])
    assert e.value.code == capi.ERR_UNSUPPORTED and "deeper" in e.value.text
    bufs = []
    try:                                                  # again, to look at the image the refused call leaves
        j = capi.InpaintJob()
        j.H, j.W, j.radius = 1, 4097, 5
        j.image, _s, ibuf, _r = padded(ctx, img, 0, 0, bufs)
        j.fill, _s, _b, _r = padded(ctx, np.where(F, 255, 0).astype(np.uint8), 0, 0, bufs)
        bufs += [ctx.alloc(ctx.mask_inpaint_scratch([j])), ctx.alloc(4)]
        with pytest.raises(capi.Gs360Error):
            ctx.mask_inpaint_dev([j], bufs[2], bufs[3])
        assert np.array_equal(ctx.download(ibuf, (1, 4097, 3), np.uint8), img)
    finally:
        for b in bufs:
            ctx.free(b)


@pytest.mark.parametrize("shadow", [False, True])
def test_the_public_chain_equals_the_restatements(ctx, shadow):
    """finish_with_inpaint: the finishing chain (after the shadow estimate or not) with kind mask and invert off, then the inpaint,
    all on the device, against maskfinish_np / maskshadow_np and the inpaint restatement"""
    photos = [maskshadow_cases.photograph(97, 130, 12), maskshadow_cases.photograph(64, 80, 13, False)]
    images, raws = [p[0] for p in photos], [p[1] for p in photos]
    params = maskshadow_cases.CHAIN_PARAMS
    outs, K = maskfinish.finish_with_inpaint(ctx, raws, params, None, images, maskshadow_cases.CHAIN_SHADOW if shadow else None)
    for img, raw, out, k in zip(images, raws, outs, K):
        if shadow:
            mask, _n = maskshadow_np.finish_with_shadow(img, raw, params, maskshadow_cases.CHAIN_SHADOW, None, "mask", False)
        else:
            mask, _n = maskfinish_np.finish(raw, params, None, None, "mask", False)
        exp, Kw = ref.inpaint(img, mask > 0)
        print(f"shadow {shadow}: {int((mask > 0).sum())} pixels of F, K {int(k)} (restatement {Kw}), {int((out != exp).any(axis=2).sum())} pixels differ")
        assert int(k) == Kw and np.array_equal(out, exp)
    assert K[0] > 0 and K[1] == 0 and np.array_equal(outs[1], images[1])


def test_limits_and_argument_errors_on_the_argument_path(ctx):
    buf, levels = ctx.alloc(4096), ctx.alloc(4)

    def job(H=8, W=8, radius=5, **kw):
        j = capi.InpaintJob()
        j.H, j.W, j.radius, j.image, j.fill = H, W, radius, buf.ptr, buf.ptr
        for k, v in kw.items():
            setattr(j, k, v)
        return j
    try:
        for j in (job(32769, 8), job(8, 32769), job(radius=2), job(radius=1), job(radius=9)):
            with pytest.raises(capi.Gs360Error) as e:
                ctx.mask_inpaint_scratch([j])
            assert e.value.code == capi.ERR_UNSUPPORTED
            with pytest.raises(capi.Gs360Error) as e:
                ctx.mask_inpaint_dev([j], buf, levels)
            assert e.value.code == capi.ERR_UNSUPPORTED
        for j in (job(H=0), job(radius=0), job(image=None), job(fill=None), job(image_stride=23), job(fill_stride=7)):
            with pytest.raises(capi.Gs360Error) as e:
                ctx.mask_inpaint_dev([j], buf, levels)
            assert e.value.code == capi.ERR_ARG
        with pytest.raises(capi.Gs360Error) as e:         # a scratch that is too small
            ctx.mask_inpaint_dev([job(64, 64)], buf, levels)
        assert e.value.code == capi.ERR_ARG
        assert ctx.mask_inpaint_scratch([job(32768, 32768)]) > 12 * 2 ** 30 and ctx.mask_inpaint_scratch([]) == 0
    finally:
        ctx.free(buf)
        ctx.free(levels)
