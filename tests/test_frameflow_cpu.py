"""FS-FLOW v1 without a GPU: hand-derivable answers of the NumPy restatement (tests/frameflow_np.py), the host logic of
gs360.frameflow (geometry, record values, the chain of _compute_flow_magnitudes) and the agreement of header, binding and
exports."""
import ctypes
import math
import pathlib
import re

import numpy as np
import pytest

import frameflow_np as fnp
from conftest import ROOT
from gs360 import capi, frameflow


def _blocks(rng, H, W, block=6):
    g = np.repeat(np.repeat(rng.integers(0, 256, (H // block + 2, W // block + 2)), block, 0), block, 1)
    return np.clip(g + rng.integers(-3, 4, g.shape), 0, 255).astype(np.uint8)


def _value(a, b, crop=1.0, mode="none"):
    return fnp.flow_values([a, b], [(0, 1)], crop, mode)[0]


def test_identical_frames_give_exactly_zero():
    rng = np.random.default_rng(1)
    a = _blocks(rng, 160, 320)[:160, :320]
    assert _value(a, a) == 0.0


def test_flat_frame_has_no_corners():
    a = np.full((120, 200), 77, np.uint8)
    assert len(fnp.Frame(a, frameflow.flow_geometry(120, 200, 1.0), False).corners) == 0
    assert _value(a, a) is None


def test_whole_pixel_shift_recovers_its_length():
    rng = np.random.default_rng(2)
    big = _blocks(rng, 200, 360)
    a = big[20:180, 20:340]
    b = big[22:182, 17:337]      # content moves by (+3, -2)
    v = _value(a, b)
    assert abs(v - math.hypot(3, 2)) < 0.1


def test_isolated_squares_give_their_corners_five_pixels_apart():
    g = np.zeros((80, 80), np.uint8)
    g[20:40, 20:40] = 200
    g[50:53, 50:53] = 200        # 3 x 3: its corners are closer than 5 pixels to each other
    c = fnp.Frame(g, frameflow.flow_geometry(80, 80, 1.0), False).corners
    pts = {tuple(map(int, p)) for p in c}
    for want in ((20, 20), (39, 20), (20, 39), (39, 39)):
        assert any(abs(x - want[0]) <= 3 and abs(y - want[1]) <= 3 for x, y in pts), (want, pts)   # the 7 x 7 block peaks just inside
    d2 = ((c[:, None, :] - c[None, :, :]) ** 2).sum(-1) + np.eye(len(c)) * 1e9
    assert d2.min() >= 25
    assert sum(1 for x, y in pts if 48 <= x <= 54 and 48 <= y <= 54) <= 2


def test_noise_frame_is_capped_at_1000_corners():
    rng = np.random.default_rng(3)
    n = rng.integers(0, 256, (320, 320), dtype=np.uint8)
    keys = fnp.candidates(fnp.min_eig(n), None)
    assert len(keys) > 3000
    assert len(fnp.select(keys, 320, 320)) == 1000


@pytest.mark.parametrize("H, W, levels", [(320, 320, 3), (64, 64, 3), (60, 60, 2), (40, 40, 2), (30, 100, 1), (12, 9, 1)])
def test_tiny_frames_use_fewer_pyramid_levels(H, W, levels):
    assert len(fnp.pyramid(np.zeros((H, W), np.uint8))) == levels


def test_pyr_down_of_a_constant_is_the_constant_and_sizes_round_up():
    d = fnp.pyr_down(np.full((17, 33), 91, np.uint8))
    assert d.shape == (9, 17) and (d == 91).all()


def test_border_is_reflect_101_at_any_distance():
    assert [fnp.border(i, 3) for i in range(-5, 8)] == [1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1]
    assert fnp.border(-15, 1) == 0


def test_geometry_follows_the_reference_expressions():
    assert frameflow.flow_geometry(4320, 7680, 0.6) == (1536, 864, 4608, 2592, 320, 180)
    assert frameflow.flow_geometry(3840, 3840, 1.0) == (0, 0, 3840, 3840, 320, 320)
    assert frameflow.flow_geometry(200, 300, 0.6) == (60, 40, 180, 120, 180, 120)
    assert frameflow.flow_geometry(1, 1, 0.6) == (0, 0, 1, 1, 1, 1)
    assert frameflow.area_fast_factors(3840, 3840, 320, 320) == (12, 12)
    assert frameflow.area_fast_factors(4608, 2592, 320, 180) is None


def test_area_fast_path_equals_block_means_rounded_half_to_even():
    g = np.array([[1, 2, 3, 4], [1, 2, 3, 5]], np.uint8)      # block sums 6 and 15 -> 1.5 -> 2, 3.75 -> 4
    assert fnp.area_fast(g, 2, 2).tolist() == [[2, 4]]
    g = np.array([[0, 1, 2, 3]], np.uint8)                    # 0.5 -> 0, 2.5 -> 2
    assert fnp.area_fast(g, 2, 1).tolist() == [[0, 2]]


def test_area_general_path_of_an_integer_factor_matches_the_fast_path_on_smooth_data():
    rng = np.random.default_rng(4)
    g = rng.integers(0, 256, (24, 36)).astype(np.uint8)
    assert np.abs(fnp.area_general(g, 12, 8).astype(int) - fnp.area_fast(g, 3, 3).astype(int)).max() <= 1


def test_value_of_records():
    assert frameflow.value_of((0, 0, 0.0)) is None
    assert frameflow.value_of((5, 0, 0.0)) is None
    assert frameflow.value_of((5, 4, 2.0)) == 0.5
    assert frameflow.value_of((5, 4, float("inf"))) is None


def test_flow_magnitudes_chain_semantics(monkeypatch, tmp_path):
    """In-place max on both frames of a pair, 9999.0 for a None pair, a missing record breaks the chain, the count of pairs."""
    files = []
    for k in range(6):
        p = tmp_path / f"{k}.png"
        if k != 3:
            p.write_bytes(b"x")
        files.append(str(p))
    vals = {("0", "1"): 1.5, ("1", "2"): None, ("4", "5"): 0.25}

    def fake_chunk(ctx, records, chunk, images):
        per = [[vals[(pathlib.Path(records[l]["file_paths"][0]).stem, pathlib.Path(records[r]["file_paths"][0]).stem)]]
               for l, r in chunk]
        return {}, per, [True] * len(chunk)
    monkeypatch.setattr(frameflow, "_chunk_values", fake_chunk)
    monkeypatch.setattr(frameflow.framescore, "default_context", lambda: None)
    monkeypatch.setattr(frameflow, "_decode", lambda p: None)
    records = [{"file_paths": [f]} for f in files]
    arr = [0.0, 3.0, 0.0, 0.0, 0.0, 0.0]
    n = frameflow._compute_flow_magnitudes(records, arr, 0.6, 2, "Optical flow")
    assert n == 3
    assert arr == [1.5, 9999.0, 9999.0, 0.0, 0.25, 0.25]
    assert frameflow._compute_flow_magnitudes(records[:1], arr, 0.6, 2, "x") == 0


def test_record_magnitude_rejects_unequal_paths():
    assert frameflow._compute_record_flow_magnitude({"file_paths": ["a"]}, {"file_paths": ["a", "b"]}, 1.0) is None
    assert frameflow._compute_record_flow_magnitude({"file_paths": []}, {"file_paths": []}, 1.0) is None


def test_16_bit_frames_are_unsupported():
    with pytest.raises(capi.Gs360Error) as e:
        frameflow.flow_arrays(None, [np.zeros((8, 8), np.uint16)] * 2, [(0, 1)], 1.0)
    assert e.value.code == -4


def test_header_binding_and_exports_agree():
    h = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "gs360.h").read_text(), flags=re.S)
    assert "gs360_frame_flow_u8" in capi.EXPORTS
    assert re.search(r"#define GS360_FLOW_MAX_SIDE (\d+)", h).group(1) == str(capi.FLOW_MAX_SIDE) == str(frameflow.FLOW_DOWNSCALE)
    assert re.search(r"#define GS360_FLOW_MAX_CORNERS (\d+)", h).group(1) == str(capi.FLOW_MAX_CORNERS)
    assert ctypes.sizeof(capi.FrameFlow) == 24 and ctypes.sizeof(capi.FlowPoint) == 24
    assert frameflow.RECORD_DTYPE.itemsize == 24 and frameflow.POINT_DTYPE.itemsize == 24
    m = re.search(r"typedef struct gs360_frame_flow \{(.*?)\} gs360_frame_flow;", h, re.S).group(1)
    assert re.findall(r"\w+(?=[,;])", m) == [n for n, _ in capi.FrameFlow._fields_]
    m = re.search(r"typedef struct gs360_flow_point \{(.*?)\} gs360_flow_point;", h, re.S).group(1)
    assert re.findall(r"\w+(?=[,;])", m) == [n for n, _ in capi.FlowPoint._fields_]


def test_errors_without_a_gpu():
    """The entry point validates its arguments before it touches a device; on a machine without one the library reports it."""
    L = capi.load_library()
    assert hasattr(L, "gs360_frame_flow_u8")
    rc = L.gs360_frame_flow_u8(None, None, 0, 8, 8, 3, 0, 0, 0, 0, 8, 8, 8, 8, 0, None, 1, None, None, 0)
    assert rc != 0 and "ctx" in capi.last_error(L)
