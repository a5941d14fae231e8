"""-m gpu: gs360_MaskFinish end to end.  A folder of three images, raw masks for two of them and one shared manual layer: every mode's
files carry the reference's names and decode to the restatement's pixels (tests/maskfinish_np.py), the log lines are the
reference's, and with GS360_PNG_ENCODER=device the files are the device PNG encoder's with the same pixels."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG
from gs360 import imageio, maskfinish

import maskfinish_np as ref

pytestmark = pytest.mark.gpu
TOOL = [sys.executable, str(PKG / "cli_tools" / "gs360_MaskFinish.py")]
H, W = 48, 70
PARAMS = maskfinish.Params(close=5, expand_pixels=4, edge_fuse_pixels=6, thresh=127)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """-> (root, {stem: (image, raw mask or None, add layer or None)})"""
    root = tmp_path_factory.mktemp("maskfinish")
    for d in ("in", "raw", "paint"):
        (root / d).mkdir()
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[:H, :W]
    disc = (((yy - 20) ** 2 + (xx - 30) ** 2 <= 64) * 255).astype(np.uint8)
    gray = np.where(rng.random((H, W)) < 0.02, 200, rng.integers(0, 128, (H, W))).astype(np.uint8)    # 200 is set, < 128 is not
    small = np.zeros((24, 35), np.uint8)                 # another size: resized with NEAREST
    small[2:6, 30:35] = 255
    add = np.zeros((H, W), np.uint8)
    add[40:44, 5:25] = 255
    content = {"shot_0001_A": (disc, add), "shot_0002_B": (gray, None), "plain": (None, None), "shot_0003_A": (small, add)}
    data = {}
    for stem, (raw, layer) in content.items():
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        imageio.write_image(root / "in" / f"{stem}.png", img)
        if raw is not None:
            imageio.write_image(root / "raw" / f"{stem}.png", raw)
            if raw.shape != (H, W):
                from PIL import Image
                raw = np.array(Image.fromarray(raw).resize((W, H), Image.NEAREST))
        data[stem] = (img, raw, layer)
    imageio.write_image(root / "paint" / "view__A__add.png", add)
    return root, data


def run_tool(root, out, mode, encoder=None, extra=()):
    env = {k: v for k, v in os.environ.items() if k != "GS360_PNG_ENCODER"}
    if encoder:
        env["GS360_PNG_ENCODER"] = encoder
    r = subprocess.run(TOOL + ["-i", str(root / "in"), "--raw-mask-dir", str(root / "raw"), "--manual-mask-dir", str(root / "paint"),
                               "-o", str(out), "--mode", mode, "--mask-expand-pixels", "4", "--edge-fuse-pixels", "6", *extra],
                       capture_output=True, text=True, timeout=300, env=env)
    return r.returncode, r.stdout, r.stderr


NAMES = {"mask": "{}.png", "alpha": "{}.png", "cutout": "{}_cutout.png", "keep_person": "{}_keep_person.png",
         "remove_person": "{}_remove_person.png"}
KINDS = {"mask": ("mask", True), "alpha": ("rgba", True), "cutout": ("rgba", False), "keep_person": ("keep", False),
         "remove_person": ("remove", False)}


def check_files(out, data, mode):
    assert sorted(p.name for p in out.iterdir()) == sorted(NAMES[mode].format(stem) for stem in data)
    kind, invert = KINDS[mode]
    for stem, (img, raw, layer) in data.items():
        want, _n = ref.finish(raw, PARAMS, layer, img, kind, invert, (H, W))
        got = imageio.read_image(out / NAMES[mode].format(stem))
        assert np.array_equal(got if got.shape[2] > 1 else got[:, :, 0], want), (mode, stem)


@pytest.mark.parametrize("mode", list(NAMES))
def test_every_modes_files_decode_to_the_restatements_pixels(folder, tmp_path, mode):
    root, data = folder
    rc, out, err = run_tool(root, tmp_path / "out", mode)
    assert rc == 0, out + err
    assert out.splitlines()[:3] == ["Mask expand: 4 px", "Edge fuse: 6 px", f"Manual mask dir: {root / 'paint'}"]
    check_files(tmp_path / "out", data, mode)


def test_the_device_png_encoder_writes_the_same_pixels(folder, tmp_path):
    root, data = folder
    rc, out, err = run_tool(root, tmp_path / "dev", "alpha", encoder="device")
    assert rc == 0, out + err
    check_files(tmp_path / "dev", data, "alpha")


def test_an_edge_fuse_wider_than_an_image_is_one_err_line(folder, tmp_path):
    root, _data = folder
    rc, out, _err = run_tool(root, tmp_path / "out", "mask", extra=("--edge-fuse-pixels", "49"))
    assert rc == 1 and [ln for ln in out.splitlines() if ln.startswith("[ERR] ")] == [out.splitlines()[-1]]
    assert not (tmp_path / "out").exists() or not list((tmp_path / "out").iterdir())


def test_a_refusal_about_a_later_image_writes_nothing(tmp_path):
    """every image is looked at before the first device call: the second image's shorter side is below --edge-fuse-pixels"""
    for d in ("in", "raw"):
        (tmp_path / d).mkdir()
    imageio.write_image(tmp_path / "in" / "a.png", np.zeros((H, W, 3), np.uint8))
    imageio.write_image(tmp_path / "in" / "b.png", np.zeros((20, 30, 3), np.uint8))
    r = subprocess.run(TOOL + ["-i", str(tmp_path / "in"), "--raw-mask-dir", str(tmp_path / "raw"), "-o", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=300)
    lines = r.stdout.splitlines()
    assert r.returncode == 1 and lines[-1].startswith("[ERR] ") and sum(ln.startswith("[ERR] ") for ln in lines) == 1
    assert not (tmp_path / "out").exists() or not list((tmp_path / "out").iterdir())
