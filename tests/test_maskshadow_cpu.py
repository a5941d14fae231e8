"""MSK-SHADOW v1 without a GPU: the host tables and size rules of gs360/maskfinish.py, and the restatement (tests/maskshadow_np.py)
against brute force and hand-counted shapes."""
import numpy as np
import pytest

from gs360 import maskfinish

import maskshadow_cases as cases
import maskshadow_np as ref


def test_gaussian_weights():
    for sigma, ksize in ((21, 169), (2, 17)):
        w = maskfinish.gaussian_weights(sigma)
        assert w.dtype == np.float32 and len(w) == ksize
        assert np.array_equal(w, w[::-1])
        assert abs(float(w.astype(np.float64).sum()) - 1.0) < 1e-6
        assert w[ksize // 2] == w.max() and (np.diff(w[ksize // 2:]) < 0).all()
    with pytest.raises(ValueError):
        maskfinish.gaussian_weights(0)


def test_saturation_divisors():
    t = maskfinish.sat_div_table()
    assert t.dtype == np.int32 and len(t) == 256 and t[0] == 0 and t[1] == 1044480 and t[255] == 4096
    px = np.array([[[255, 0, 0], [90, 90, 90], [0, 0, 0], [10, 200, 30]]], np.uint8)
    S = ref.saturation(px)[0]
    assert S[0] == 255 and S[1] == 0 and S[2] == 0
    assert S[3] == (190 * int(t[200]) + 2048) >> 12


@pytest.mark.parametrize("count, k, close_k", [(0, 25, 5), (1, 25, 5), (16899, 25, 5), (16900, 27, 5), (409600, 129, 27), (10 ** 9, 129, 27)])
def test_shadow_sizes_at_the_breakpoints(count, k, close_k):
    assert maskfinish.shadow_sizes(count, 25) == (k, close_k)


def test_shadow_sizes_follow_near_px():
    assert maskfinish.shadow_sizes(100, 2) == (3, 5)
    assert maskfinish.shadow_sizes(100, 200) == (201, 41)


def brute_reflect(p, n):
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * (n - 1) - p
    return p


@pytest.mark.parametrize("n", [1, 2, 3])
def test_reflect_101_repeats_on_sides_below_the_radius(n):
    r = 8
    p = np.arange(-r, n + r)
    assert ref.reflect101(p, n).tolist() == [brute_reflect(int(v), n) for v in p]


@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (3, 2), (5, 9)])
def test_the_filter_against_loops(shape):
    rng = np.random.default_rng(7)
    v = rng.integers(0, 256, shape).astype(np.float32)
    half = maskfinish.gaussian_weights(2)[8:]
    r = len(half) - 1

    def one(vals, n, c):
        s = np.float32(half[0]) * vals[c]
        for i in range(1, r + 1):
            s = np.float32(s + np.float32(half[i] * np.float32(vals[brute_reflect(c - i, n)] + vals[brute_reflect(c + i, n)])))
        return s
    H, W = shape
    rows = np.array([[one(v[y], W, x) for x in range(W)] for y in range(H)], np.float32)
    both = np.array([[one(rows[:, x], H, y) for x in range(W)] for y in range(H)], np.float32)
    assert np.array_equal(ref.blur(v, half), both)


def area2_of(X, min_area=1):
    G, clean, areas = ref.component_filter(X, min_area)
    return G, clean, areas


def plane(H, W, *boxes):
    X = np.zeros((H, W), bool)
    for y0, x0, y1, x1 in boxes:
        X[y0:y1, x0:x1] = True
    return X


def test_area_of_lines_rectangles_and_an_l():
    for n in (1, 2, 9):
        assert area2_of(plane(7, 12, (3, 1, 4, 1 + n)))[2] == [0]
        assert area2_of(plane(12, 7, (1, 3, 1 + n, 4)))[2] == [0]
    for a, b in ((2, 2), (3, 5), (6, 4)):
        assert area2_of(plane(9, 9, (1, 2, 1 + a, 2 + b)))[2] == [2 * (a - 1) * (b - 1)]
    L = plane(5, 5, (1, 1, 3, 2), (2, 1, 3, 3))
    assert L.sum() == 3 and area2_of(L)[2] == [1]


def test_a_line_is_dropped_and_a_rectangle_kept():
    X = plane(10, 20, (1, 1, 2, 19), (4, 2, 8, 7))
    _G, clean, areas = area2_of(X, 1)
    assert areas == [0, 24] and np.array_equal(clean, plane(10, 20, (4, 2, 8, 7)))


def test_a_ring_counts_as_its_rectangle_and_its_hole_is_filled_with_what_lies_in_it():
    X = np.zeros((14, 16), bool)
    cases.ring(X, 2, 3, 12, 13, 1)
    X[6:8, 7:9] = True                                    # a component inside the hole: swallowed
    G, clean, areas = area2_of(X, 1)
    assert areas == [2 * 9 * 9]
    assert np.array_equal(G, plane(14, 16, (2, 3, 12, 13))) and np.array_equal(clean, G)


def test_a_c_that_opens_onto_the_border_is_not_filled():
    X = np.zeros((12, 12), bool)
    X[0:8, 2] = X[0:8, 8] = True
    X[7, 2:9] = True
    G, _clean, _areas = area2_of(X)
    assert np.array_equal(G, X)
    X[0, 2:9] = True                                      # closed along the border line itself: now it is a ring
    assert ref.outer_filled(X)[3, 5]


def test_a_diagonal_step_joins_two_blobs():
    X = plane(10, 10, (1, 1, 4, 4), (4, 4, 7, 7))
    _G, clean, areas = area2_of(X, 8)
    assert areas == [8 + 8]                               # one component: two 3 x 3 blobs; the step's cell has two corners and adds 0
    assert np.array_equal(clean, X)
    apart = plane(10, 10, (1, 1, 4, 4), (5, 4, 8, 7))
    assert area2_of(apart, 8)[2] == [8, 8]


def test_the_thresholds_two_components():
    X = cases.label_planes(97, 130)["threshold"]
    _G, clean, areas = area2_of(X, cases.LABEL_MIN_AREA)
    assert areas == [39, 40]
    assert clean[12, 12] and not clean[32, 12] and clean.sum() == 30


def test_the_label_fixtures_say_what_their_names_say():
    for H, W in cases.LABEL_SIZES[:1]:
        P = cases.label_planes(H, W)
        G, _c, areas = area2_of(P["spiral"])
        assert len(areas) == 1 and 0 < areas[0] <= H and np.array_equal(G, P["spiral"])     # one half cell per turn
        G, _c, areas = area2_of(P["checkerboard"])
        assert len(areas) == 1 and G[1:-1, 1:-1].all()
        G, _c, areas = area2_of(P["rings"])
        assert len(areas) == 1 and np.array_equal(G, plane(H, W, (3, 3, H - 3, W - 3)))
        G, _c, areas = area2_of(P["open-cs"])
        assert len(areas) == 5 and (G & ~P["open-cs"]).sum() == 14 * 26
        assert not area2_of(P["empty"])[0].any() and area2_of(P["full"])[2] == [2 * (H - 1) * (W - 1)]


def test_the_photograph_exercises_every_branch():
    """what tests/test_maskshadow_gpu.py relies on, asserted on the restatement"""
    img, raw, sat = cases.photograph(200, 333, 11)
    r = ref.shadow(img, raw, cases.CHAIN_PARAMS, cases.CHAIN_SHADOW)
    th2 = 2 * cases.CHAIN_SHADOW.min_area
    assert 0 < r["clean"].sum() < 0.5 * r["clean"].size
    assert any(a < th2 for a in r["areas"]) and any(a >= th2 for a in r["areas"])
    assert (r["G"] & ~r["C2"]).any()                      # a hole is filled
    assert not r["C0"][sat].any()
    import dataclasses
    loose = ref.shadow(img, raw, cases.CHAIN_PARAMS, dataclasses.replace(cases.CHAIN_SHADOW, sat_max=255))
    assert loose["C0"][sat].all()                         # ... rejected by its saturation alone
    none = ref.shadow(img, None, cases.CHAIN_PARAMS, cases.CHAIN_SHADOW, (200, 333))
    assert not none["M"].any() and none["count"] == 0
