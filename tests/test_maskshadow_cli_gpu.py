"""-m gpu: gs360_MaskFinish --include_shadow end to end.  With GS360_MASK_SHADOW=device the files of a folder of two images are the
library call's (maskfinish.finish_with_shadow, itself checked against the restatement in tests/test_maskshadow_gpu.py); without the
variable the flag ends the run with the line it always did, and a 16-bit image is refused before anything is written."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG
from gs360 import imageio, maskfinish

import maskshadow_cases as cases

pytestmark = pytest.mark.gpu
TOOL = [sys.executable, str(PKG / "cli_tools" / "gs360_MaskFinish.py")]
PARAMS = maskfinish.Params(close=5, expand_pixels=4, edge_fuse_pixels=6, thresh=127)
REFUSAL = "[ERR] --include_shadow is not built: the contour-filtered shadow estimate is not part of this tool"


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """-> (root, {stem: (image, raw mask)})"""
    root = tmp_path_factory.mktemp("maskshadow")
    (root / "in").mkdir()
    (root / "raw").mkdir()
    data = {}
    for stem, args in (("walk_0001", (97, 130, 12)), ("walk_0002", (120, 90, 14))):
        img, raw, _sat = cases.photograph(*args)
        imageio.write_image(root / "in" / f"{stem}.png", img)
        imageio.write_image(root / "raw" / f"{stem}.png", raw)
        data[stem] = (img, raw)
    return root, data


def run_tool(root, out, mode, shadow_env, indir="in"):
    env = {k: v for k, v in os.environ.items() if k not in ("GS360_MASK_SHADOW", "GS360_PNG_ENCODER")}
    if shadow_env:
        env["GS360_MASK_SHADOW"] = shadow_env
    r = subprocess.run(TOOL + ["-i", str(root / indir), "--raw-mask-dir", str(root / "raw"), "-o", str(out), "--mode", mode,
                               "--mask-expand-pixels", "4", "--edge-fuse-pixels", "6", "--include_shadow"],
                       capture_output=True, text=True, timeout=300, env=env)
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("mode, kind, invert, suffix", [("mask", "mask", True, ""), ("cutout", "rgba", False, "_cutout")])
def test_the_files_are_the_library_calls(ctx, folder, tmp_path, mode, kind, invert, suffix):
    root, data = folder
    rc, out, err = run_tool(root, tmp_path / "out", mode, "device")
    assert rc == 0, out + err
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == sorted(f"{stem}{suffix}.png" for stem in data)
    stems = sorted(data)
    outs, counts = maskfinish.finish_with_shadow(ctx, [data[s][1] for s in stems], PARAMS, None, None, [data[s][0] for s in stems],
                                                 kind=kind, invert=invert)
    plain, _n = maskfinish.finish(ctx, [data[s][1] for s in stems], PARAMS, None, [data[s][0] for s in stems], kind=kind, invert=invert)
    for stem, want, without in zip(stems, outs, plain):
        got = imageio.read_image(tmp_path / "out" / f"{stem}{suffix}.png")
        assert np.array_equal(got if got.shape[2] > 1 else got[:, :, 0], want), (mode, stem)
        assert not np.array_equal(want, without), (stem, "the shadow changed nothing")
    assert (counts > 0).all()


@pytest.mark.parametrize("env", [None, "off"])
def test_without_the_variable_the_flag_is_refused_as_before(folder, tmp_path, env):
    root, _data = folder
    rc, out, _err = run_tool(root, tmp_path / "out", "mask", env)
    assert rc == 1 and out.splitlines() == [REFUSAL]
    assert not (tmp_path / "out").exists()


def test_an_unknown_value_of_the_variable_is_one_err_line(folder, tmp_path):
    root, _data = folder
    rc, out, _err = run_tool(root, tmp_path / "out", "mask", "host")
    assert rc == 1 and len(out.splitlines()) == 1 and out.startswith("[ERR] GS360_MASK_SHADOW must be off or device")


def test_a_16_bit_image_is_refused_before_anything_is_written(folder, tmp_path):
    root, _data = folder
    (root / "deep").mkdir(exist_ok=True)
    imageio.write_image(root / "deep" / "a.png", np.zeros((40, 50, 3), np.uint8))
    imageio.write_image(root / "deep" / "b.png", np.zeros((40, 50), np.uint16))
    rc, out, _err = run_tool(root, tmp_path / "out", "mask", "device", indir="deep")
    assert rc == 1 and out.splitlines()[-1] == "[ERR] b.png: 16-bit images are not built for --include_shadow"
    assert not (tmp_path / "out").exists() or not list((tmp_path / "out").iterdir())
