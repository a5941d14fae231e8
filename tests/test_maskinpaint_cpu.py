"""MSK-INPAINT v1 on the CPU: the restatement (tests/maskinpaint_np.py) against brute force and against itself, and the host side of
gs360/maskfinish.py.  The spec's own fixture: 48 x 40, a disc of radius 9, a 12 x 12 block in the bottom-right corner and a 3-row
strip on the top edge."""
import numpy as np
import pytest

from gs360 import maskfinish

import maskinpaint_np as ref

F = ref.fixture_mask()
H, W = F.shape
RAMPS = {"constant": (0, 0, 93), "2x+10": (2, 0, 10), "3y+5": (0, 3, 5), "2x+3y+7": (2, 3, 7), "250-2x-3y": (-2, -3, 250)}


def brute_d2(mask):
    oy, ox = np.nonzero(~mask)
    yy, xx = np.mgrid[:mask.shape[0], :mask.shape[1]]
    d2 = ((yy[:, :, None] - oy) ** 2 + (xx[:, :, None] - ox) ** 2).min(axis=2)
    return np.where(mask, d2, 0)


def test_the_fixture_is_the_specs():
    L, _T, K = ref.prepare(F)
    assert (W, H) == (48, 40) and int(F.sum()) == 418 and K == 12 and (L[~F] == 0).all() and (L[F] >= 1).all()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_d2_and_levels_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    masks = [F, rng.random((23, 31)) < 0.8, rng.random((1, 40)) < 0.9, rng.random((37, 1)) < 0.9]
    blob = np.ones((30, 26), bool)
    blob[rng.integers(0, 30), rng.integers(0, 26)] = False           # a single pixel outside F
    for mask in masks + [blob]:
        want = brute_d2(mask)
        assert np.array_equal(ref.distance2(mask), want)
        L = ref.levels(want)
        k = np.ceil(np.sqrt(want.astype(np.float64))).astype(np.int64)   # exact in double at this size
        assert np.array_equal(L, k)
    assert np.array_equal(ref.levels(np.array([0, 1, 2, 4, 5, 9, 10, 4095 ** 2, 4095 ** 2 + 1])), [0, 1, 2, 2, 3, 3, 4, 4095, 4096])


def test_the_offset_table():
    offs = ref.offsets(5)
    assert len(offs) == 80 and len(ref.offsets(8)) == 196 and len(ref.offsets(3)) == 28
    assert [(dy, dx) for dy, dx, _r, _i in offs] == sorted((dy, dx) for dy, dx, _r, _i in offs)      # row-major
    assert offs[0][:2] == (-5, 0) and (0, 0) not in [(dy, dx) for dy, dx, _r, _i in offs]
    for dy, dx, rlen, inv2 in offs:
        assert 0 < dy * dy + dx * dx <= 25
        assert rlen == np.float32(np.sqrt(np.float64(dy * dy + dx * dx))) and inv2 == np.float32(1.0 / (dy * dy + dx * dx))
    pairs, rlen, inv2 = maskfinish.inpaint_offsets(5)
    assert pairs.dtype == np.int32 and rlen.dtype == inv2.dtype == np.float32
    assert [tuple(p) for p in pairs] == [o[:2] for o in offs]
    assert np.array_equal(rlen, [o[2] for o in offs]) and np.array_equal(inv2, [o[3] for o in offs])
    for bad in (0, 2, 9):
        with pytest.raises(ValueError):
            maskfinish.inpaint_offsets(bad)


@pytest.mark.parametrize("name", list(RAMPS))
def test_a_constant_and_the_ramps_are_reproduced(name):
    """integer slopes make every gradient exact: zero wrong bytes; without the image-gradient term the ramps are not reproduced"""
    img = ref.ramp(H, W, *RAMPS[name])
    holed = img.copy()
    holed[F] = 0
    out, K = ref.inpaint(holed, F)
    assert K == 12 and np.array_equal(out, img)
    if name != "constant":
        flat, _K = ref.inpaint(holed, F, use_gradient=False)
        wrong = (flat != img).any(axis=2)
        assert wrong.sum() > 300 and not wrong[~F].any()


def test_the_level_at_once_restatement_equals_the_loop():
    img = ref.photograph(H, W, 5)
    a, Ka = ref.inpaint(img, F)
    b, Kb = ref.inpaint_loop(img, F)
    assert Ka == Kb == 12 and np.array_equal(a, b)
    assert np.array_equal(a[~F], img[~F]) and (a[F] != img[F]).any()


def test_noise_clamps_at_both_ends_and_leaves_the_outside_alone():
    rng = np.random.default_rng(9)
    img = rng.choice(np.array([0, 255], np.uint8), size=(H, W, 3))
    out, _K = ref.inpaint(img, F)
    assert np.array_equal(out[~F], img[~F])
    assert (out[F] == 0).any() and (out[F] == 255).any()


def test_full_and_empty_masks_leave_the_image_alone():
    img = ref.photograph(12, 9, 1)
    for mask in (np.zeros((12, 9), bool), np.ones((12, 9), bool)):
        out, K = ref.inpaint(img, mask)
        assert K == 0 and np.array_equal(out, img)
        out, K = ref.inpaint_loop(img, mask)
        assert K == 0 and np.array_equal(out, img)


def test_a_region_deeper_than_4095_levels_is_refused():
    mask = np.ones((1, 4200), bool)
    mask[0, 0] = False
    with pytest.raises(ValueError):
        ref.prepare(mask)
    assert ref.prepare(mask[:, :4096])[2] == 4095


def test_the_environment_switch(monkeypatch):
    monkeypatch.delenv("GS360_MASK_INPAINT", raising=False)
    assert maskfinish.inpaint_mode_from_env() is False
    monkeypatch.setenv("GS360_MASK_INPAINT", "off")
    assert maskfinish.inpaint_mode_from_env() is False
    monkeypatch.setenv("GS360_MASK_INPAINT", "device")
    assert maskfinish.inpaint_mode_from_env() is True
    monkeypatch.setenv("GS360_MASK_INPAINT", "telea")
    with pytest.raises(ValueError, match="GS360_MASK_INPAINT must be off or device"):
        maskfinish.inpaint_mode_from_env()
