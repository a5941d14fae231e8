"""FS-FFT v1 without a GPU: the NumPy restatement (tests/framescore_fft_np.py) against the reference's fft_energy through the host
mask path, finish() on a gs360_frame_fft record against finish() on the planes, the kernel's half-spectrum crediting, the ctypes
mirror of the record and the `fft` keyword of the score_* functions."""
import ctypes
import pathlib
import subprocess
import tempfile

import numpy as np
import pytest

import framescore_fft_np as ffnp
import framescore_np as fnp
from conftest import ROOT
from gs360 import capi, framescore

FLAGS = [0, capi.FS_CIRCLE, capi.FS_HIGHLIGHTS, capi.FS_CIRCLE | capi.FS_HIGHLIGHTS]
SIZES = [(204, 512), (409, 512), (512, 409), (7, 9), (8, 10), (9, 8), (1, 16), (16, 1), (1, 1), (17, 3), (127, 509)]


def _planes(rng, h, w, kind="photo"):
    """(g float32, gray at the nearest sample) of an h x w fft input: smooth gradients, an edge, highlights and mild noise."""
    yy, xx = np.mgrid[:h, :w]
    if kind == "constant":
        g = np.full((h, w), 97.25, np.float32)
    elif kind == "noise":
        g = rng.uniform(0, 255, size=(h, w)).astype(np.float32)
    else:
        g = 60 + 0.3 * xx + 0.2 * yy + np.where(xx > w / 2, 70, 0) + rng.normal(0, 2, size=(h, w))
        g = np.where((xx - w / 3) ** 2 + (yy - h / 2) ** 2 < (min(h, w) / 4) ** 2, 250, g)
        g = np.clip(g, 0, 255).astype(np.float32)
    near = np.clip(np.round(g + rng.integers(-2, 3, size=(h, w))), 0, 255).astype(np.float32)
    return g, near


def _geometry(h, w):
    H, W = 2 * h + 3, 3 * w + 1
    return H, W, framescore.band_rows(H, 0.8)


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("kind", ["photo", "noise", "constant"])
def test_restatement_equals_the_reference_fft_energy(h, w, flags, kind):
    rng = np.random.default_rng(h * 1000 + w + flags)
    g, near = _planes(rng, h, w, kind)
    H, W, band = _geometry(h, w)
    rec = ffnp.fft_record(g, near, H, W, band, flags)
    assert rec["n"] == h * w
    mask = ffnp.host_mask(near, H, W, band, "fisheye_circle" if flags & capi.FS_CIRCLE else "none", bool(flags & capi.FS_HIGHLIGHTS))
    assert rec["n_valid"] == int(mask.sum())
    for masked, g_mask in ((False, None), (True, mask)):
        got = framescore.fft_energy_from_record(rec, masked)
        want = framescore.fft_energy(g, g_mask)
        assert got == pytest.approx(want, rel=2e-6, abs=1e-9), (masked, got, want)


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("flags", FLAGS)
def test_half_spectrum_crediting_covers_every_position_once(h, w, flags):
    rng = np.random.default_rng(h + 7 * w)
    g, near = _planes(rng, h, w, "noise")
    H, W, band = _geometry(h, w)
    full = ffnp.fft_record(g, near, H, W, band, flags)
    half = ffnp.half_spectrum_record(g, near, H, W, band, flags)
    assert half["n_valid"] == full["n_valid"] and half["n"] == full["n"]
    for k in ("sum_hf", "sum_hf_valid"):
        assert half[k] == pytest.approx(full[k], rel=1e-12, abs=1e-9), k


def _frame(rng, H, W, kind):
    if kind == "white":
        return np.full((H, W, 3), 255, np.uint8)
    yy, xx = np.mgrid[:H, :W]
    g = (xx * 7 + yy * 3) % 256
    g = np.where((xx - W / 3) ** 2 + (yy - H / 2) ** 2 < (min(H, W) / 4) ** 2, 250, g)
    g = np.clip(g + rng.integers(-3, 4, size=g.shape), 0, 255).astype(np.uint8)
    return np.repeat(g[:, :, None], 3, axis=2) ^ np.arange(3, dtype=np.uint8) * 17


FINISH_CASES = [  # H, W, kind, crop, mask_mode, ignore_highlights
    (60, 90, "structured", 0.8, "none", False), (60, 90, "structured", 0.8, "none", True),
    (61, 61, "structured", 0.8, "fisheye_circle", False), (61, 61, "structured", 0.6, "fisheye_circle", True),
    (700, 300, "structured", 0.8, "fisheye_circle", True),      # a 300 x 560 band: resized fft input of 274 x 512
    (40, 70, "white", 0.8, "fisheye_circle", True),             # every valid pixel is a highlight: empty mask, mean branch
    (40, 70, "white", 0.8, "none", True),                       # p255 = 1: no mask at all
]


@pytest.mark.parametrize("H,W,kind,crop,mask_mode,hl", FINISH_CASES)
@pytest.mark.parametrize("metric", ["fft", "hybrid", "lapvar"])
def test_finish_on_a_record_equals_finish_on_the_planes(H, W, kind, crop, mask_mode, hl, metric):
    rng = np.random.default_rng(H + W)
    img = _frame(rng, H, W, kind)
    band = framescore.band_rows(H, crop)
    st = fnp.frame_stats(img, *band, mask_mode == "fisheye_circle", hl)
    g, near = fnp.fft_input(img, *band)
    flags = (capi.FS_CIRCLE if mask_mode == "fisheye_circle" else 0) | (capi.FS_HIGHLIGHTS if hl else 0)
    rec = ffnp.fft_record(g, near, H, W, band, flags)
    want = framescore.finish(st, H, W, band, metric, True, hl, mask_mode, (g, near))
    got = framescore.finish(st, H, W, band, metric, True, hl, mask_mode, fft_rec=rec)
    assert len(got) == 9
    for k, (a, b) in enumerate(zip(got, want)):
        if k in (0, 7) and metric != "lapvar":
            assert a == pytest.approx(b, rel=2e-6, abs=1e-9), k
        else:
            assert a == b, k
    if kind == "white" and mask_mode == "fisheye_circle":
        assert rec["n_valid"] == 0


def test_frame_fft_layout_matches_the_header():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "gs360.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %d\n", sizeof(gs360_frame_fft), offsetof(gs360_frame_fft, sum_hf), offsetof(gs360_frame_fft, sum_hf_valid),
           offsetof(gs360_frame_fft, n_valid), offsetof(gs360_frame_fft, n), GS360_FFT_MAX_SIDE);
    return 0;
}'''
    with tempfile.TemporaryDirectory() as td:
        src = pathlib.Path(td) / "t.c"
        src.write_text(prog)
        exe = pathlib.Path(td) / "t"
        subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
        out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    F = capi.FrameFft
    assert out[:5] == [ctypes.sizeof(F), F.sum_hf.offset, F.sum_hf_valid.offset, F.n_valid.offset, F.n.offset] == [32, 0, 8, 16, 24]
    assert framescore.FFT_DTYPE.itemsize == 32 and list(framescore.FFT_DTYPE.names) == [n for n, _ in F._fields_]
    assert out[5] == capi.FFT_MAX_SIDE == framescore.FFT_LONG_SIDE


def test_unknown_fft_mode_is_a_value_error(tmp_path):
    img = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(ValueError):
        framescore.score_arrays(None, [img], "hybrid", 0.8, True, False, fft="bogus")
    with pytest.raises(ValueError):
        framescore.score_files([str(tmp_path / "x.png")], "hybrid", 0.8, 0, True, False, fft="bogus")
    with pytest.raises(ValueError):
        framescore.score_one_file(str(tmp_path / "x.png"), "hybrid", 0.8, 0, True, False, fft="gpu")
    with pytest.raises(ValueError):
        framescore.score_one_record({"file_paths": [str(tmp_path / "x.png")]}, "fft", 0.8, 0, True, False, fft="Device")
    assert framescore.DEFAULT_FFT == "host" and framescore.fft_mode(None) == "host" and framescore.fft_mode("device") == "device"
