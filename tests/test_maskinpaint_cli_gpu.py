"""-m gpu: gs360_MaskFinish --mode inpaint end to end.  With GS360_MASK_INPAINT=device the `<stem>_inpaint.png` files of a folder of
three images hold the restatements' bytes (tests/maskfinish_np.py for the mask, tests/maskinpaint_np.py for the fill), through the
host writer and through the device PNG encoder; an image without a detection comes out unchanged.  Without the variable the mode ends
the run with the line it always did; a bad value and a 16-bit image are one [ERR] line each, before anything is written."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG
from gs360 import imageio, maskfinish

import maskfinish_np
import maskinpaint_np as ref
import maskshadow_cases as cases

pytestmark = pytest.mark.gpu
TOOL = [sys.executable, str(PKG / "cli_tools" / "gs360_MaskFinish.py")]
PARAMS = maskfinish.Params(close=5, expand_pixels=4, edge_fuse_pixels=6, thresh=127)
REFUSAL = "[ERR] --mode inpaint is not built: Telea inpainting is not part of this tool"


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """-> (root, {stem: (image, raw mask or None)}); walk_0003 has no raw mask: nothing detected"""
    root = tmp_path_factory.mktemp("maskinpaint")
    (root / "in").mkdir()
    (root / "raw").mkdir()
    data = {}
    for stem, args in (("walk_0001", (97, 130, 12)), ("walk_0002", (120, 90, 14)), ("walk_0003", (40, 50, 15))):
        img, raw, _sat = cases.photograph(*args)
        imageio.write_image(root / "in" / f"{stem}.png", img)
        if stem != "walk_0003":
            imageio.write_image(root / "raw" / f"{stem}.png", raw)
        data[stem] = (img, raw if stem != "walk_0003" else None)
    return root, data


def run_tool(root, out, env_value, extra=(), indir="in", png=None, shadow=None):
    env = {k: v for k, v in os.environ.items() if k not in ("GS360_MASK_INPAINT", "GS360_MASK_SHADOW", "GS360_PNG_ENCODER")}
    for key, value in (("GS360_MASK_INPAINT", env_value), ("GS360_PNG_ENCODER", png), ("GS360_MASK_SHADOW", shadow)):
        if value:
            env[key] = value
    r = subprocess.run(TOOL + ["-i", str(root / indir), "--raw-mask-dir", str(root / "raw"), "-o", str(out), "--mode", "inpaint",
                               "--mask-expand-pixels", "4", "--edge-fuse-pixels", "6"] + list(extra),
                       capture_output=True, text=True, timeout=300, env=env)
    return r.returncode, r.stdout, r.stderr


@pytest.fixture(scope="module")
def expected(folder):
    """the restatements' files, computed once"""
    _root, data = folder
    out = {}
    for stem, (img, raw) in data.items():
        mask, _n = maskfinish_np.finish(raw, PARAMS, None, None, "mask", False, shape=img.shape[:2])
        out[stem] = ref.inpaint(img, mask > 0)
    return out


@pytest.mark.parametrize("png", [None, "device"])
def test_the_files_hold_the_restatements_bytes(folder, expected, tmp_path, png):
    root, data = folder
    rc, out, err = run_tool(root, tmp_path / "out", "device", png=png)
    assert rc == 0, out + err
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == sorted(f"{stem}_inpaint.png" for stem in data)
    for stem, (img, _raw) in data.items():
        got = imageio.read_image(tmp_path / "out" / f"{stem}_inpaint.png")
        want, K = expected[stem]
        assert np.array_equal(got, want), (stem, int((got != want).any(axis=2).sum()))
        assert (K > 0 and not np.array_equal(want, img)) or stem == "walk_0003"
    assert np.array_equal(expected["walk_0003"][0], data["walk_0003"][0])      # an empty mask: the image as it was


def test_the_shadow_estimate_composes_in_front(ctx, folder, expected, tmp_path):
    root, data = folder
    rc, out, err = run_tool(root, tmp_path / "out", "device", extra=["--include_shadow"], shadow="device")
    assert rc == 0, out + err
    stems = sorted(data)
    outs, K = maskfinish.finish_with_inpaint(ctx, [data[s][1] if data[s][1] is not None else data[s][0].shape[:2] for s in stems], PARAMS,
                                             None, [data[s][0] for s in stems], shadow=True)
    for stem, want in zip(stems, outs):
        assert np.array_equal(imageio.read_image(tmp_path / "out" / f"{stem}_inpaint.png"), want), stem
    assert not np.array_equal(outs[0], expected[stems[0]][0]), "the shadow changed nothing"
    assert K[0] > 0 and K[2] == 0


@pytest.mark.parametrize("env", [None, "off"])
def test_without_the_variable_the_mode_is_refused_as_before(folder, tmp_path, env):
    root, _data = folder
    rc, out, _err = run_tool(root, tmp_path / "out", env)
    assert rc == 1 and out.splitlines() == [REFUSAL]
    assert not (tmp_path / "out").exists()


def test_an_unknown_value_of_the_variable_is_one_err_line(folder, tmp_path):
    root, _data = folder
    rc, out, _err = run_tool(root, tmp_path / "out", "telea")
    assert rc == 1 and len(out.splitlines()) == 1 and out.startswith("[ERR] GS360_MASK_INPAINT must be off or device")
    assert not (tmp_path / "out").exists()


def test_a_16_bit_image_is_refused_before_anything_is_written(folder, tmp_path):
    root, _data = folder
    (root / "deep").mkdir(exist_ok=True)
    imageio.write_image(root / "deep" / "a.png", np.zeros((40, 50, 3), np.uint8))
    imageio.write_image(root / "deep" / "b.png", np.zeros((40, 50), np.uint16))
    rc, out, _err = run_tool(root, tmp_path / "out", "device", indir="deep")
    assert rc == 1 and out.splitlines()[-1] == "[ERR] b.png: 16-bit images are not built for --mode inpaint"
    assert not (tmp_path / "out").exists() or not list((tmp_path / "out").iterdir())
