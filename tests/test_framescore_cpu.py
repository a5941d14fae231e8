"""Frame sharpness scoring without a GPU: known answers of the FS-SPEC v1 restatement (tests/framescore_np.py), the host finish
layer of gs360.framescore, hybrid_scores, and the C-ABI declaration / binding / layout of gs360_frame_stats_u8."""
import ctypes
import math
import pathlib
import re
import subprocess
import tempfile
import threading

import numpy as np
import pytest

import framescore_np as fnp
import gs360
from conftest import ROOT
from gs360 import capi, frameflow, framescore

HEADER = (ROOT / "include" / "gs360.h").read_text()


# ---- the restatement ------------------------------------------------------------------------------------------------------
def test_impulse_gives_the_ksize3_laplacian_taps():
    img = np.zeros((5, 5), np.uint8)
    img[2, 2] = 100
    lap, gx, gy = fnp.laplacian_sobel(fnp.gray_u8(img))
    assert lap[2, 2] == -800
    assert [lap[1, 1], lap[1, 3], lap[3, 1], lap[3, 3]] == [200] * 4
    assert lap[1, 2] == lap[2, 1] == 0                       # the ksize-1 kernel would put 100 here
    st = fnp.frame_stats(img, 0, 5)
    assert (st["sum_lap"], st["sum_lap2"]) == (0, 800 ** 2 + 4 * 200 ** 2)
    assert gx[2, 1] == 200 and gx[1, 1] == 100 and gy[1, 2] == 200 and gy[3, 3] == -100
    assert st["sum_mag2"] == 2 * (4 * 100 ** 2 + 2 * 200 ** 2)


def test_band_is_reflected_at_its_own_edges():
    rows = np.array([200, 0, 10, 50, 0, 200], np.uint8)
    img = np.repeat(rows[:, None], 4, axis=1)
    st = fnp.frame_stats(img, 2, 4)
    # band rows [10, 50]: above 10 is 50 and below 50 is 10 (reflect-101 inside the band, not the frame's rows 0 / 0)
    assert st["sum_lap"] == 4 * (320 - 320)
    assert st["sum_lap2"] == 8 * 320 ** 2
    assert st["sum_mag2"] == 0 and st["n"] == 8 and st["sum_gray"] == 4 * 60
    one = fnp.frame_stats(img, 3, 4)                          # a 1-row band reflects onto itself
    assert one["sum_lap"] == one["sum_lap2"] == one["sum_mag2"] == 0


def test_highlight_threshold_is_243():
    img = np.array([[242, 243, 255, 0]], np.uint8)
    st = fnp.frame_stats(img, 0, 1, highlights_on=True)
    assert st["n_highlight"] == 2 and st["n_valid"] == 2 and st["sum_gray_valid"] == 242


def test_gray_constants_and_channel_order():
    px = np.array([[[10, 200, 30, 99]]], np.uint8)
    assert fnp.gray_u8(px[:, :, :3], 0)[0, 0] == (10 * 4899 + 200 * 9617 + 30 * 1868 + 8192) >> 14
    assert fnp.gray_u8(px, 2)[0, 0] == (30 * 4899 + 200 * 9617 + 10 * 1868 + 8192) >> 14


@pytest.mark.parametrize("H,W", [(5, 5), (4, 4), (6, 9), (9, 6), (1, 1), (2, 1), (7, 2)])
def test_circle_in_integers_equals_the_reference_float_form(H, W):
    yy, xx = np.ogrid[:H, :W]
    r = max(1.0, min(W, H) * 0.5)
    ref = (xx - (W - 1) * 0.5) ** 2 + (yy - (H - 1) * 0.5) ** 2 <= r * r
    assert np.array_equal(fnp.circle(H, W), ref)
    assert np.array_equal(framescore.circle_mask(H, W, np.arange(H), np.arange(W)), ref)


def test_circle_known_counts():
    assert int(fnp.circle(5, 5).sum()) == 21          # radius 2.5 about the centre pixel
    assert int(fnp.circle(4, 4).sum()) == 12          # radius 2 about a corner point: the four corners are out


@pytest.mark.parametrize("H,crop,want", [
    (5, 0.8, (0, 4)), (5, 0.6, (1, 4)), (5, 1.0, (0, 5)), (3840, 0.8, (384, 3456)), (3840, 0.6, (768, 3072)),
    (3840, 1.0, (0, 3840)), (2880, 0.8, (288, 2592)), (2880, 0.6, (576, 2304)), (2880, 1.0, (0, 2880)),
    (1, 0.8, (0, 1)), (1, 0.6, (0, 1)), (1, 1.0, (0, 1))])
def test_band_rows(H, crop, want):
    assert framescore.band_rows(H, crop) == want


@pytest.mark.parametrize("crop", [0.0, -0.5, 1.5])
def test_crop_outside_the_unit_interval_is_a_value_error(crop):
    with pytest.raises(ValueError):
        framescore.band_rows(100, crop)


def test_inter_area_restatement():
    a = np.arange(16, dtype=np.float32).reshape(4, 4)
    assert np.array_equal(fnp.inter_area(a, 2, 2), [[2.5, 4.5], [10.5, 12.5]])     # integral factors: block means
    assert np.array_equal(fnp.inter_area(a, 4, 4), a)                               # equal sizes: the image itself
    row = np.array([[3.0, 6.0, 9.0]], np.float32)                                   # 3 -> 2: weights (2/3, 1/3), (1/3, 2/3)
    np.testing.assert_allclose(fnp.inter_area(row, 2, 1), [[4.0, 8.0]], rtol=1e-6)
    assert framescore.fft_input_size(7680, 3072) == (512, 204)
    assert framescore.fft_input_size(300, 200) == (300, 200)
    assert list(framescore.nearest_index(2, 5)) == [0, 2]


# ---- the host finish layer ------------------------------------------------------------------------------------------------
def _st(**kw):
    st = dict(n_circle=16, n_highlight=0, n_highlight_in_circle=0, n=4, sum_gray=400, sum_lap=8, sum_lap2=80, sum_mag2=1000,
              n_valid=2, sum_gray_valid=60, sum_lap_valid=2, sum_lap2_valid=10, sum_mag2_valid=90)
    st.update(kw)
    return st


FLAT = (np.full((4, 4), 7, np.float32), np.full((4, 4), 7, np.float32))   # a flat fft input: every high frequency is 0


def test_finish_per_metric_unmasked():
    band = (0, 4)
    # var = 80/4 - (8/4)^2 = 16; tenengrad = 1000/4 = 250; brightness = 400/4/255
    assert framescore.finish(_st(), 4, 4, band, "lapvar", False, False, "none") == (16.0, 0.0, 0.0, 100 / 255, 1.0, 256.0, None, None, 1.0)
    assert framescore.finish(_st(), 4, 4, band, "tenengrad", False, False, "none") == (250.0, 0.0, 0.0, 100 / 255, 1.0, None, 250.0, None, 1.0)
    assert framescore.finish(_st(), 4, 4, band, "fft", False, False, "none", FLAT) == (0.0, 0.0, 0.0, 100 / 255, 1.0, None, None, 0.0, 1.0)
    got = framescore.finish(_st(), 4, 4, band, "hybrid", True, False, "none", FLAT)
    motion = 1.0 - 0.4 * (1.0 - 250.0 / 5250.0)
    assert got == ((0.6 * 256.0 + 0.3 * 250.0 + 0.1 * 0.0) * motion, 0.0, 0.0, 100 / 255, 1.0, 256.0, 250.0, 0.0, motion)
    assert framescore.finish(_st(), 4, 4, band, "sharpness?", False, False, "none") == framescore.FAILED


def test_finish_hybrid_dark_penalty():
    got = framescore.finish(_st(sum_gray=4 * 51), 4, 4, (0, 4), "hybrid", False, False, "none", FLAT)   # brightness 0.2
    assert got[3] == 0.2 and got[4] == 1.0 - 0.5 * (1.0 - 0.2 / 0.35) and got[8] == 1.0


def test_finish_circle_uses_the_valid_sums_and_falls_back_when_empty():
    got = framescore.finish(_st(), 4, 4, (0, 4), "lapvar", False, False, "fisheye_circle")
    # valid: mean 2/2 = 1, var = 10/2 - 1 = 4; brightness = 60 * (1/2) / 255
    assert got[0] == 4.0 and got[5] == 16.0 and got[3] == 30 / 255
    got = framescore.finish(_st(n_valid=0, sum_gray_valid=0, sum_lap_valid=0, sum_lap2_valid=0, sum_mag2_valid=0), 4, 4, (0, 4),
                            "lapvar", False, False, "fisheye_circle")
    assert got[0] == 16.0 and got[3] == 100 / 255


def test_finish_highlight_branches():
    H = W = 4
    # no circle, 0 < p255 < 1: the ~highlight mask applies
    got = framescore.finish(_st(n_highlight=4), H, W, (0, 4), "tenengrad", False, True, "none")
    assert got[2] == 0.25 and got[0] == 45.0
    # p255 == 1: the reference drops the mask (FS:957-958) -> all band pixels
    got = framescore.finish(_st(n_highlight=16), H, W, (0, 4), "tenengrad", False, True, "none")
    assert got[2] == 1.0 and got[0] == 250.0
    # p255 == 0: no mask either
    got = framescore.finish(_st(), H, W, (0, 4), "tenengrad", False, True, "none")
    assert got[2] == 0.0 and got[0] == 250.0
    # circle: p255 over the circle, mask = circle & ~highlight whatever p255 is
    got = framescore.finish(_st(n_circle=12, n_highlight=5, n_highlight_in_circle=3), H, W, (0, 4), "tenengrad", False, True,
                            "fisheye_circle")
    assert got[2] == 0.25 and got[0] == 45.0


def test_hybrid_scores():
    t = [(None, 0.0, 0.0, 0.5, 1.0, 100.0, 10.0, 1.0, 1.0),
         (None, 0.0, 0.0, 0.5, 1.0, 300.0, 30.0, 3.0, 0.5),
         (None, 0.0, 0.0, 0.5, 1.0, 200.0, 20.0, 3.0, 1.0),
         (7.0, 0.0, 0.0, 0.5, 1.0, None, None, None, 1.0)]
    assert framescore.hybrid_scores(t) == [0.0, (0.6 * 1.0 + 0.3 * 1.0 + 0.1 * 1.0) * 0.5, 0.6 * 0.5 + 0.3 * 0.5 + 0.1 * 1.0, 7.0]
    same = [(1.0, 0.0, 0.0, 0.5, 1.0, 5.0, 5.0, 5.0, 1.0)] * 3       # isclose(vmax, vmin) -> every feature normalises to 0
    assert framescore.hybrid_scores(same) == [0.0, 0.0, 0.0]


def test_unsupported_sources_fail_before_any_gpu_work():
    with pytest.raises(gs360.Gs360Error) as e:
        framescore.score_arrays(None, [np.zeros((4, 4, 3), np.uint16)], "lapvar", 0.8, False, False)
    assert e.value.code == -4
    with pytest.raises(ValueError):
        framescore.score_arrays(None, [np.zeros((4, 4, 3), np.uint8)], "lapvar", 1.5, False, False)
    with pytest.raises(gs360.Gs360Error):
        framescore.score_one_file("x.png", "lapvar", 0.8, 640, False, False)


def test_unreadable_file_gives_the_reference_failure_tuple(tmp_path):
    assert framescore.score_one_file(str(tmp_path / "missing.png"), "hybrid", 0.8, 0, True, False) == \
        (None, 0.0, 0.0, 0.0, 1.0, None, None, None, 1.0)


# ---- DeviceFrames keep their own row stride -------------------------------------------------------------------------------
class _Buf:
    def __init__(self, ptr, nbytes):
        self.ptr, self.nbytes = ptr, nbytes


class _RecordingCtx:
    """A context without a device: it records (pointers, stride) of every frame_*_dev call and answers every download with
    records of ones (zeros would divide by n = 0 in the finish layer) or, for bytes, zeros."""

    def __init__(self):
        self.slot_locks = [threading.Lock()]
        self.launches = []
        self.next_ptr = 0x1000

    def alloc(self, nbytes):
        self.next_ptr += 0x100000
        return _Buf(self.next_ptr, int(nbytes))

    def to_device(self, array):
        return self.alloc(np.ascontiguousarray(array).nbytes)

    def free(self, buf):
        pass

    def download(self, buf, shape, dtype=np.uint8):
        return np.zeros(shape, dtype) if np.dtype(dtype) == np.uint8 else np.ones(shape, dtype)

    def _launch(self, frames, H, W, Cn, stride):
        self.launches.append(([b.ptr for b in frames], int(stride) or W * Cn))

    def frame_stats_dev(self, frames, H, W, Cn, band, stats, stride=0, **kw):
        self._launch(frames, H, W, Cn, stride)

    def frame_edge_dev(self, frames, H, W, Cn, band, out, red_index=0, stride=0, slot=0):
        self._launch(frames, H, W, Cn, stride)

    def frame_flow_dev(self, frames, H, W, Cn, crop, small_w, small_h, pairs, out, stride=0, **kw):
        self._launch(frames, H, W, Cn, stride)
        self.launches[-1] += ([tuple(p) for p in pairs],)


def _mixed_stride_frames(ctx, H, W, Cn):
    """Six DeviceFrames of one shape whose strides are 0, W*C and W*C + 8, interleaved, and {pointer: normalised stride}."""
    frames = [framescore.DeviceFrame(ctx.alloc(H * (W * Cn + 8)), H, W, Cn, s) for s in (0, W * Cn, W * Cn + 8, 0, W * Cn + 8, W * Cn)]
    return frames, {fr.buf.ptr: fr.stride or W * Cn for fr in frames}


def _assert_own_strides(ctx, own, W, Cn):
    """Every launch reads each DeviceFrame with that frame's stride (0 and W*C are the same) and each uploaded copy packed."""
    for launch in ctx.launches:
        for p in launch[0]:
            want = own.get(p, W * Cn)
            assert launch[1] == want, f"frame at {p:#x} launched with stride {launch[1]}, its own is {want}"


def test_device_frames_of_one_shape_are_launched_with_their_own_strides():
    H, W, Cn = 61, 90, 3
    for run in (lambda c, fr: framescore.score_arrays(c, fr, "lapvar", 0.8, False, True),
                lambda c, fr: framescore.edge_arrays(c, fr, 0.8)):
        ctx = _RecordingCtx()
        frames, own = _mixed_stride_frames(ctx, H, W, Cn)
        assert len(run(ctx, frames)) == len(frames)
        _assert_own_strides(ctx, own, W, Cn)
        assert sorted(p for launch in ctx.launches for p in launch[0]) == sorted(own)      # every frame once, none copied
        assert [len(launch[0]) for launch in ctx.launches] == [2, 1, 1, 1, 1]              # runs of one stride: 0 and W*C share
    ctx = _RecordingCtx()
    frames, own = _mixed_stride_frames(ctx, H, W, Cn)
    pairs = [(0, 1), (1, 2), (2, 0), (2, 4), (3, 5), (4, 4)]
    recs = frameflow.flow_records(ctx, frames, pairs, 1.0)
    assert len(recs) == len(pairs)
    _assert_own_strides(ctx, own, W, Cn)
    assert sum(len(launch[2]) for launch in ctx.launches) == len(pairs)                    # every pair ran, once
    by_ptrs = {tuple(launch[0]): launch for launch in ctx.launches}
    # pairs of one stride stay on the device: (0,1) and (3,5) together (0 = W*C), (2,4) and (4,4) together
    assert by_ptrs[tuple(frames[k].buf.ptr for k in (0, 1, 3, 5))][2] == [(0, 1), (2, 3)]
    assert by_ptrs[tuple(frames[k].buf.ptr for k in (2, 4))][2] == [(0, 1), (1, 1)]


def test_device_frames_refuses_a_mixture_of_strides():
    ctx = _RecordingCtx()
    frames, _ = _mixed_stride_frames(ctx, 8, 10, 1)
    with pytest.raises(ValueError):
        with framescore.device_frames(ctx, frames):
            pass
    with framescore.device_frames(ctx, frames[:2] + [np.zeros((8, 10), np.uint8)]) as (bufs, stride, _alloc):
        assert len(bufs) == 3 and stride in (0, 10)
    with framescore.device_frames(ctx, [frames[2], frames[4]]) as (bufs, stride, _alloc):
        assert stride == 18


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_frame_stats_entry_point_is_declared_bound_and_exported():
    assert re.search(r"^int gs360_frame_stats_u8\(", HEADER, flags=re.M)
    assert "gs360_frame_stats_u8" in capi.EXPORTS
    lib = ctypes.CDLL(str(capi.LIB_PATH))
    assert hasattr(lib, "gs360_frame_stats_u8")
    assert gs360.load_library().gs360_frame_stats_u8.argtypes is not None


def test_frame_stats_struct_layout_matches_the_header():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "gs360.h"
int main(void) {
    printf("%zu %zu %zu %zu %u %u\n", sizeof(gs360_frame_stats), offsetof(gs360_frame_stats, n),
           offsetof(gs360_frame_stats, n_valid), offsetof(gs360_frame_stats, sum_mag2_valid), GS360_FS_CIRCLE, GS360_FS_HIGHLIGHTS);
    return 0;
}'''
    with tempfile.TemporaryDirectory() as td:
        src = pathlib.Path(td) / "t.c"
        src.write_text(prog)
        exe = pathlib.Path(td) / "t"
        subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
        out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = capi.FrameStats
    assert out == [ctypes.sizeof(S), S.n.offset, S.n_valid.offset, S.sum_mag2_valid.offset, capi.FS_CIRCLE, capi.FS_HIGHLIGHTS]
    assert out[0] == 104 and list(framescore.FIELDS) == list(fnp.FIELDS)


def test_module_imports_without_torch():
    import importlib
    import sys
    mod = importlib.import_module("gs360.framescore")
    assert callable(mod.score_one_file) and callable(mod.score_one_record) and callable(mod.score_files)
    text = pathlib.Path(mod.__file__).read_text()
    assert "torch" not in text and "oracle" not in text
    assert math.isfinite(mod.HYBRID_DARK_THRESHOLD) and "framescore" in sys.modules["gs360.framescore"].__name__
