"""The three MaskFinish stages past their own tiles and at the limits the C ABI accepts, on the device: masks and images wider than a
workgroup's 1024 pixels of a row and than the row blur's 2048 outputs, the largest structuring element (1025 x 1025, p = 512), the
largest blur radius (255: the column pass's 163 328 bytes of dynamic LDS), side strips of seven dwords, and one inpaint level longer
than a workgroup from a single region across the row tile seam.  The helpers and the comparisons are those of test_maskfinish_gpu.py,
test_maskshadow_gpu.py and test_maskinpaint_gpu.py: no byte differs from the NumPy restatements, and the guards, the row padding and
the scratch guard stay untouched.  The fixtures are maskfinish_cases.limit_cases(), maskshadow_cases.blur_limit_jobs() and the
labelling planes at maskshadow_cases.LABEL_WIDE; the same ones go through the sanitized host checks on the CPU."""
import numpy as np
import pytest

from gs360 import capi, maskfinish

import maskinpaint_np
import maskshadow_cases
import test_maskfinish_gpu as finish
import test_maskinpaint_gpu as inpaint
import test_maskshadow_gpu as shadow

pytestmark = pytest.mark.gpu

LIMITS = finish.LIMITS
BLUR = maskshadow_cases.blur_limit_jobs()                # the Gaussian fixtures and their two-tap twins, as jobs
SEAM = 1024                                              # the first tile seam of the pack, pixel, count, select, output and morph kernels
FILL_GROUP = 256                                         # listed pixels of a workgroup of the inpaint's fill; its row tile is as wide


# ---- the finishing chain ---------------------------------------------------------------------------------------------------------
def assert_neither_saturates(names):
    """the restatement's finished mask has 5 % .. 95 % of its pixels set, and set and clear ones on both sides of the seam"""
    for name in names:
        out, count = finish.want(name)                   # kind mask, inverted: 0 where the mask is set
        B = out == 0
        assert count == int(B.sum())
        print(f"{name}: {B.mean():.4f} set; {B[:, :SEAM].mean():.4f} left of x = {SEAM}, {B[:, SEAM:].mean():.4f} from it on")
        assert 0.05 <= B.mean() <= 0.95, name
        for side in (B[:, :SEAM], B[:, SEAM:]):
            assert side.any() and not side.all(), name


def test_the_limit_fixtures_in_one_call(ctx):
    """140 x 1700 under a 1025 x 1025 ellipse (halo 18, 16 bands, both morph tile columns), 33 x 2100 (three pack, count and output
    tile columns, 65 dword seams), 210 x 1100 with strips 200 wide (seven dwords a row, spread over 141 rows)"""
    names = list(LIMITS)
    assert names == ["140x1700-p512", "33x2100-corners", "210x1100-f200"]
    assert_neither_saturates(names)
    finish.check(names, finish.run_finish(ctx, names))


def test_three_tile_columns_composed_from_padded_rows_and_an_offset_base(ctx):
    """kind rgba with invert on: the byte path of the 4-byte group load in tile columns 1 and 2, one pixel per lane of the compose"""
    names = ["33x2100-corners"]
    finish.check(names, finish.run_finish(ctx, names, kind="rgba", invert=True, pad=11, offset=7), kind="rgba", invert=True)


def test_the_largest_element_alone(ctx):
    """the expand step and nothing else, one job per call: a failure names the morph kernel.  (The fixture's own parameters are the
    step's, so the restatement is the one the batch above is compared with.)"""
    name = "140x1700-p512"
    c = LIMITS[name]
    step = maskfinish.Params(close=1, expand_pixels=maskfinish.MAX_EXPAND, edge_fuse_pixels=0)
    assert c.params == step and c.add is None and 2 * step.expand_pixels + 1 == capi.MASK_MAX_ELEMENT
    finish.check([name], finish.run_finish(ctx, [name]))


# ---- the shadow estimate ---------------------------------------------------------------------------------------------------------
def blur_jobs(names):
    jobs = [(n, BLUR[n]) for n in names]
    for name, job in jobs:
        C0 = shadow.want(name, job)["C0"]
        print(f"{name}: r {len(job.half) - 1}, {int(C0.sum())} of {C0.size} pixels in C0")
        assert C0.any() and not C0.all(), name
    return jobs


@pytest.mark.parametrize("name", list(BLUR))
def test_blur_past_a_row_segment_and_at_the_largest_radius(ctx, name):
    """40 x 2100 at r = 84: the row pass's second segment (52 outputs, reflection at the right edge from x0 = 2048), H below r, three
    pixel and select tile columns.  150 x 70 at r = 255: the column launch with the most dynamic LDS the call can ask for, two column
    tiles each way, both sides below r.  9 x 2100 at r = 255: a full row segment's last staged float.  The -ends twins put the whole
    weight on the two outermost taps, so that the ends of every staged row and column decide the bits"""
    assert len(maskfinish.gaussian_weights(63.75)) == 2 * capi.SHADOW_MAX_RADIUS + 1
    wide = BLUR[name].raw.shape[1] > 2048
    assert len(BLUR[name].half) - 1 == (84 if name.startswith("40x2100") else capi.SHADOW_MAX_RADIUS)
    jobs = blur_jobs([name])
    shadow.check(jobs, shadow.run_shadow(ctx, jobs, pad=13 if wide else 0, offset=5 if wide else 0))


def test_three_radii_in_one_launch(ctx):
    """the column launch's LDS is sized by the largest radius among its jobs while every job indexes it by its own: r = 255, r = 84
    and a one-tap filter (r = 0) in one pair of calls"""
    H, W = maskshadow_cases.LABEL_SIZES[0]
    jobs = blur_jobs(["150x70-s63.75", "40x2100-s21-sign"])
    jobs.append((f"{H}x{W}-seams", maskshadow_cases.label_job("seams", maskshadow_cases.label_planes(H, W)["seams"])))
    assert [len(j.half) - 1 for _n, j in jobs] == [255, 84, 0]
    shadow.check(jobs, shadow.run_shadow(ctx, jobs))


@pytest.mark.parametrize("name", maskshadow_cases.LABEL_WIDE_NAMES)
def test_labelling_past_two_tile_columns(ctx, name):
    H, W = maskshadow_cases.LABEL_WIDE
    X = maskshadow_cases.label_planes(H, W)[name]
    jobs = [(f"{H}x{W}-{name}", maskshadow_cases.wide_label_job(name, X))]
    w = shadow.want(*jobs[0])
    print(f"{jobs[0][0]}: {int(X.sum())} pixels set, {int(w['clean'].sum())} in clean")
    assert np.array_equal(w["C2"], X) and w["clean"].any()       # the near rectangles reach every column: the plane arrives as C2
    shadow.check(jobs, shadow.run_shadow(ctx, jobs, slot=1))


# ---- the inpaint -----------------------------------------------------------------------------------------------------------------
def disc60():
    return ("140x300-disc60", maskinpaint_np.photograph(140, 300, 5), maskinpaint_np.discs(140, 300, [(70, 230)], 60), 5)


@pytest.mark.parametrize("pad, offset", [(0, 0), (13, 5)])
def test_one_region_with_levels_longer_than_a_workgroup(ctx, pad, offset):
    """a disc of radius 60 over the row tile seam at x = 256: K = 61, and levels of more than 256 pixels from one job"""
    c = disc60()
    F = c[2]
    per_level = np.bincount(maskinpaint_np.prepare(F)[0][F])
    xs = np.nonzero(F.any(axis=0))[0]
    print(f"{c[0]}: {int(F.sum())} pixels of F in x = {xs.min()}..{xs.max()}, the longest level has {per_level.max()}")
    assert per_level.max() > FILL_GROUP and xs.min() < FILL_GROUP < xs.max()
    _outs, K = inpaint.check(ctx, [c], pad=pad, offset=offset, slot=1 if pad else 0)
    assert K[0] == len(per_level) - 1 > 2 * c[3]
