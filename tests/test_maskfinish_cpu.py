"""MSK-SPEC v1 on the CPU: the NumPy restatement (tests/maskfinish_np.py) against a four-loop brute force of the definition, the
structuring element's documented rows and the two consequences the edge fuse depends on, and the host rules of gs360/maskfinish.py."""
import numpy as np
import pytest

from gs360 import maskfinish

import maskfinish_cases as cases
import maskfinish_np as ref

CASES = cases.cases()


def element(kw, kh):
    rows, _anchor = maskfinish.structuring_rows(kw, kh)
    e = np.zeros((kh, kw), np.uint8)
    for i, (j1, j2) in enumerate(rows):
        e[i, j1:j2] = 1
    return e


def test_structuring_rows_is_opencvs_documented_ellipse():
    assert element(5, 5).tolist() == [[0, 0, 1, 0, 0], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [0, 0, 1, 0, 0]]
    assert element(3, 3).tolist() == [[0, 1, 0], [1, 1, 1], [0, 1, 0]]
    assert element(1, 1).tolist() == [[1]]
    assert maskfinish.structuring_rows(5, 5)[1] == (2, 2) and maskfinish.structuring_rows(6, 4)[1] == (3, 2)


def test_even_elements_are_asymmetric_about_their_anchor():
    rows, (ax, ay) = maskfinish.structuring_rows(6, 6)
    assert (ax, ay) == (3, 3) and len(rows) == 6
    assert rows[0] == (3, 4) and rows[3] == (0, 6)        # dy = -3: the centre column alone; dy = 0: the whole row


@pytest.mark.parametrize("s", [1, 2, 9, 40])
def test_a_flat_row_element_is_its_centre_and_a_flat_column_is_full(s):
    """the edge fuse as the reference RUNS: (2s+1) x 1 has r = 0, so its top and bottom seeds are not spread; 1 x (2s+1) has c = 0 and
    every row [0, 1), so its side seeds spread s rows"""
    assert element(2 * s + 1, 1).tolist() == [[0] * s + [1] + [0] * s]
    assert element(1, 2 * s + 1).tolist() == [[1]] * (2 * s + 1)


def test_resolve_expand_pixels_rounds_half_to_even():
    r = maskfinish.resolve_expand_pixels
    assert [r("pixels", v) for v in (0.5, 1.5, 2.5, 15, -3)] == [0, 2, 2, 15, 0]
    assert r("percent", 0, 1.0, (3840, 7680)) == 77                     # 76.8
    assert r("percent", 0, 1.0, (50, 250)) == 2 and r("percent", 0, 1.0, (350, 50)) == 4   # 2.5 and 3.5
    assert r("percent", 0, 1.0, None) == 0
    assert r(None, 3) == r("", 3) == r(" Pixels ", 3) == 3
    with pytest.raises(ValueError):
        r("ratio", 1)


def test_manual_key_follows_the_view_id_rule():
    k = maskfinish.manual_key
    assert k("shots/IMG_0001_A.jpg") == "view__A"
    assert k("IMG_0001_A_U.png") == "view__A_U"
    assert k("IMG_0001_12_D20.tif") == "view__12_D20"
    assert k("img_0001_b.jpg") == "view__B"              # the rule reads the stem in upper case
    assert k("holiday.jpg") == "file__holiday"
    assert k("IMG_0001_7.jpg") == "file__IMG_0001_7"     # a single digit is no view id
    assert k("x_A_D.png") == "view__A_D" and k("x_7_D.png") == "view__D" and k("x_A_U3.png") == "view__A_U3"
    assert k("x_A_UP.png") == "file__x_A_UP" and k("A.png") == "file__A" and k("_A.png") == "view__A"


def test_edge_fuse_wider_than_the_mask_is_refused():
    with pytest.raises(ValueError):
        maskfinish.build_jobs([(20, 30)], maskfinish.Params(edge_fuse_pixels=21))
    with pytest.raises(ValueError):
        ref.fuse(np.ones((20, 30), bool), 21)
    jobs, _keep = maskfinish.build_jobs([(20, 30)], maskfinish.Params(edge_fuse_pixels=20))
    assert (jobs[0].fuse, jobs[0].spread) == (20, 7)


def test_build_jobs_follows_the_chain_rules():
    jobs, _keep = maskfinish.build_jobs([(3840, 7680), (100, 50)], maskfinish.Params(close=0, expand_mode="percent", edge_fuse_pixels=0))
    assert [(j.close_kh, j.expand_kw, j.expand_kh, j.fuse) for j in jobs] == [(0, 155, 155, 0), (0, 3, 3, 0)]
    with pytest.raises(ValueError):
        maskfinish.build_jobs([(4, 4)], maskfinish.Params(), kind="inpaint")


def brute_chain_step(B, kw, kh):
    return ref.brute_morph(B, kw, kh, False), ref.brute_morph(B, kw, kh, True)


def small_masks():
    out = [(n, np.asarray(c.raw) > c.params.thresh) for n, c in CASES.items() if c.raw is not None and max(c.raw.shape) <= 16]
    rng = np.random.default_rng(7)
    out += [(f"random-{k}", rng.random((12, 12)) < (0.05, 0.3, 0.7)[k % 3]) for k in range(50)]
    return out


ELEMENTS = ((2, 2), (5, 5), (6, 6), (3, 3), (31, 31), (1, 7), (7, 1))


def test_the_restatement_equals_a_brute_force_of_the_definition():
    masks = small_masks()
    assert len(masks) >= 56
    for name, B in masks:
        for kw, kh in ELEMENTS:
            d, e = brute_chain_step(B, kw, kh)
            assert np.array_equal(ref.dilate(B, kw, kh), d), (name, kw, kh)
            assert np.array_equal(ref.erode(B, kw, kh), e), (name, kw, kh)


def test_the_edge_fuse_equals_a_brute_force_of_its_sentences():
    for name, B in small_masks():
        for f in sorted({f for f in (0, 1, 3, 5, min(B.shape)) if f <= min(B.shape)}):
            assert np.array_equal(ref.fuse(B, f), ref.brute_fuse(B, f)), (name, f)


def test_the_strip_fills_on_a_hand_made_mask():
    B = np.zeros((12, 14), bool)
    B[2, 5] = B[4, 5] = True                              # top strip (f = 3): rows 0..2 of column 5; row 3 stays clear
    B[6, 1] = True                                        # left strip: spread one row up and down, columns 0..1
    got = ref.fuse(B, 3)                                  # s = max(1, round(1.05)) = 1
    want = B.copy()
    want[0:3, 5] = True
    want[5:8, 0:2] = True
    assert np.array_equal(got, want)
    assert ref.fuse(np.zeros((5, 5), bool), 3).sum() == 0 and ref.fuse(B, 0) is B


def test_compose_takes_the_empty_mask_branches():
    img = cases.image_for((4, 6))
    empty, some = np.zeros((4, 6), bool), np.eye(4, 6, dtype=bool)
    for invert in (True, False):
        out, n = ref.compose(empty, "rgba", invert, img)
        assert n == 0 and (out[:, :, 3] == 0).all() and np.array_equal(out[:, :, :3], img)
        for kind in ("keep", "remove"):
            assert np.array_equal(ref.compose(empty, kind, invert, img)[0], img)
    assert (ref.compose(empty, "mask", True)[0] == 255).all() and (ref.compose(empty, "mask", False)[0] == 0).all()
    out, n = ref.compose(some, "rgba", True, img)
    assert n == 4 and np.array_equal(out[:, :, 3], np.where(some, 0, 255))
    assert np.array_equal(ref.compose(some, "keep", True, img)[0], img * some[:, :, None])
    assert np.array_equal(ref.compose(some, "remove", True, img)[0], img * ~some[:, :, None])


def test_every_fixture_runs_through_the_restatement():
    assert len(CASES) > 16
    for name, c in CASES.items():
        B = ref.chain(c.raw, c.params, c.add, cases.shape_of(c))
        assert B.shape == cases.shape_of(c) and B.dtype == bool, name
