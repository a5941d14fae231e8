"""-m gpu: GS360_JPEG_ENCODER=device through the gs360_DualFisheyeDistortionCalibration drop-in.  With the variable set every .jpg view and
mask the CLI writes must be the restatement of "JPG-SPEC v1, 4:2:0" (tests/jpeg420_np.py) applied to the pixels the same command writes
as PNG, in table and fused map modes, with the Annex K tables and with GS360_JPEG_HUFFMAN=optimal; stdout and file names do not change;
.png views, 16-bit pairs and runs without the variable keep the host codecs' files."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG
from gs360 import dualfisheye, fisheye as fe, imageio

import jpeg420_np as j420
from test_dualfisheye_cli import SMALL_XML, make_pairs

pytestmark = pytest.mark.gpu
EXE = [sys.executable, str(PKG / "cli_tools" / "gs360_DualFisheyeDistortionCalibration.py")]
VARS = ("GS360_JPEG_ENCODER", "GS360_JPEG_OPTIMIZE", "GS360_JPEG_HUFFMAN")
RESTART = 8                   # the restart interval of the tool's files, in 16 x 16 MCUs
SIZE = 96


def run_cli(args, out, encoder=None, huffman=None):
    """-> stdout with the run's own output folder replaced by OUT"""
    env = {k: v for k, v in os.environ.items() if k not in VARS}
    if encoder:
        env["GS360_JPEG_ENCODER"] = encoder
    if huffman:
        env["GS360_JPEG_HUFFMAN"] = huffman
    r = subprocess.run(EXE + args + ["--perspective-output-dir", str(out)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "errors=0" in r.stdout, r.stdout + r.stderr
    return r.stdout.replace(str(out), "OUT")


def same_lines(a, b):
    """two runs' stdout, equal up to the views' extension (and the order in which the worker threads finish their pairs)"""
    def norm(s):
        lines = s.replace(".png", ".EXT").replace(".jpg", ".EXT").splitlines()
        return sorted(lines[:-1]) + lines[-1:]
    return norm(a) == norm(b)


def files_of(out):
    return {str(p.relative_to(out)): p for p in sorted(out.rglob("*")) if p.is_file() and p.suffix.lower() in (".png", ".jpg")}


class Scene:
    """two 240-pixel synthetic pairs with masks and the template-style calibration; the PNG runs (the views' exact pixels) are made
    once per map mode and shared"""

    def __init__(self, root):
        self.root = root
        self.shots = root / "shots"
        make_pairs(self.shots, n=2)
        self.masks = root / "masks"
        self.masks.mkdir()
        rng = np.random.default_rng(9)
        for p in sorted(self.shots.glob("frame_*.png")):
            imageio.write_image(self.masks / p.name, (rng.random((240, 240)) > 0.3).astype(np.uint8) * 255)
        self.xml = root / "c.xml"
        self.xml.write_text(SMALL_XML)
        self._png = {}

    def args(self, mode, ext, quality=None, shots=None):
        a = ["-i", str(shots or self.shots), "-x", str(self.xml), "--interpolation", "linear", "--perspective-size", str(SIZE),
             "--perspective-ext", ext, "--workers", "2", "--mask-value", "5", "--map-mode", mode]
        if mode == "table" and shots is None:
            a += ["--mask-input-dir", str(self.masks), "--perspective-mask-ext", ext]
        if quality is not None:
            a += ["--perspective-jpeg-quality", str(quality)]
        return a

    def png(self, mode):
        """-> (stdout, {relative name: pixels}) of the default encoder's PNG run"""
        if mode not in self._png:
            out = self.root / f"png_{mode}"
            stdout = run_cli(self.args(mode, "png"), out)
            self._png[mode] = (stdout, {name: imageio.read_image(p) for name, p in files_of(out).items()})
            assert len(self._png[mode][1]) == (40 if mode == "table" else 20)       # 2 pairs x 10 views (+ masks)
        return self._png[mode]


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    return Scene(tmp_path_factory.mktemp("df_jpeg"))


def pixels_for_jpeg(a):
    return a[:, :, 0] if a.ndim == 3 and a.shape[2] == 1 else a


def check_run(scene, mode, quality, huffman, out):
    png_stdout, pixels = scene.png(mode)
    stdout = run_cli(scene.args(mode, "jpg", quality), out, "device", huffman)
    assert same_lines(stdout, png_stdout)                                      # the same lines, the other extension
    got = files_of(out)
    assert sorted(got) == sorted(n[:-4] + ".jpg" for n in pixels)
    restate = j420.encode_optimal if huffman == "optimal" else j420.encode
    Image = pytest.importorskip("PIL.Image")
    for name, a in pixels.items():
        data = got[name[:-4] + ".jpg"].read_bytes()
        assert data == restate(pixels_for_jpeg(a), quality, RESTART), (name, quality)
    one = Image.open(io.BytesIO(got["Images/frame_0000_A.jpg"].read_bytes()))
    assert one.size == (SIZE, SIZE) and one.mode == "RGB"
    return got


@pytest.mark.parametrize("quality", [95, 60])
@pytest.mark.parametrize("mode", ["table", "fused"])
def test_device_encoder_files_equal_the_restatement(scene, mode, quality):
    got = check_run(scene, mode, quality, None, scene.root / f"dev_{mode}_{quality}")
    if mode == "table":                                                        # masks follow the same rule: gray files, v1's bytes
        assert sum(n.startswith("Masks/") for n in got) == 20


@pytest.mark.parametrize("quality", [95, 60])
@pytest.mark.parametrize("mode", ["table", "fused"])
def test_optimal_huffman_files_equal_the_optimal_restatement(scene, mode, quality):
    check_run(scene, mode, quality, "optimal", scene.root / f"opt_{mode}_{quality}")


def test_png_views_and_unset_variable_stay_on_the_host_path(scene):
    Image = pytest.importorskip("PIL.Image")
    _stdout, pixels = scene.png("table")
    out = scene.root / "dev_png"
    run_cli(scene.args("table", "png"), out, "device")                          # .png views: the device encoder has nothing to take
    for name, p in files_of(out).items():
        assert p.read_bytes() == (scene.root / "png_table" / name).read_bytes(), name
    out = scene.root / "host_jpg"
    run_cli(scene.args("table", "jpg", 60), out)                                # variable unset: Pillow's files, as before
    got = files_of(out)
    assert len(got) == 40
    for name, a in pixels.items():
        b = io.BytesIO()
        Image.fromarray(pixels_for_jpeg(a)).save(b, "JPEG", quality=60)
        assert got[name[:-4] + ".jpg"].read_bytes() == b.getvalue(), name


def test_sixteen_bit_pairs_stay_on_the_host_path(scene):
    shots = scene.root / "shots16"
    shots.mkdir()
    rng = np.random.default_rng(15)
    for lens in "XY":
        imageio.write_image(shots / f"frame_0000_{lens}.png", rng.integers(0, 65536, (240, 240, 3), dtype=np.uint16))
    host, dev = scene.root / "host16", scene.root / "dev16"
    a = run_cli(scene.args("table", "jpg", 90, shots), host)
    b = run_cli(scene.args("table", "jpg", 90, shots), dev, "device")
    assert same_lines(a, b)
    got = files_of(dev)
    assert len(got) == 10
    for name, p in got.items():
        assert p.read_bytes() == (host / name).read_bytes(), name


def test_pair_renderer_keyword_and_counters(ctx, tmp_path):
    """render_pair's jpeg_views / jpeg_masks in process: 8-bit RGB views and gray masks come back as whole files and are counted;
    16-bit and four-channel pairs come back as arrays and jpeg_device_images stays where it was"""
    xml = tmp_path / "c.xml"
    xml.write_text(SMALL_XML)
    xml_sensors, _ = fe.load_metashape_calibration(xml)
    specs = fe.sfm10_specs(64, 14.0, "36 36", 40.0, 40.0)
    tables = fe.choose_lens_tables(xml_sensors, "0", "0", specs, 0.0, 180.0, 190.0)
    r = dualfisheye.PairRenderer(ctx, xml_sensors, specs, tables, {}, 190.0)
    rng = np.random.default_rng(21)
    kw = dict(interpolation=1, mask_outside_model=True, mask_value=5)
    try:
        assert r.stats() == {"jpeg_device_images": 0, "jpeg_device_bytes": 0}
        x, y = (rng.integers(0, 256, (240, 240, 3), dtype=np.uint8) for _ in range(2))
        mx, my = ((rng.random((240, 240)) > 0.3).astype(np.uint8) * 255 for _ in range(2))
        plain = r.render_pair(x, y, "0", "0", mask_x=mx, mask_y=my, **kw)
        assert r.stats()["jpeg_device_images"] == 0
        res = r.render_pair(x, y, "0", "0", mask_x=mx, mask_y=my, jpeg_views=(80, "standard"), jpeg_masks=(80, "optimal"), **kw)
        total = 0
        for vid, a in plain["perspective"].items():
            assert res["perspective"][vid] == j420.encode(a, 80, RESTART), vid
            assert res["masks"][vid] == j420.encode_optimal(plain["masks"][vid][:, :, 0], 80, RESTART), vid
            total += len(res["perspective"][vid]) + len(res["masks"][vid])
        assert r.stats() == {"jpeg_device_images": 20, "jpeg_device_bytes": total}
        only = r.render_pair(x, y, "0", "0", mask_x=mx, mask_y=my, jpeg_views=(80, "standard"), **kw)      # masks not asked for
        assert all(isinstance(v, bytes) for v in only["perspective"].values())
        assert all(np.array_equal(only["masks"][vid], plain["masks"][vid]) for vid in plain["masks"])
        assert r.stats()["jpeg_device_images"] == 30
        x16, y16 = (rng.integers(0, 65536, (240, 240, 3), dtype=np.uint16) for _ in range(2))
        deep = r.render_pair(x16, y16, "0", "0", jpeg_views=(80, "standard"), **kw)
        assert all(v.dtype == np.uint16 and v.shape == (64, 64, 3) for v in deep["perspective"].values())
        x4, y4 = (rng.integers(0, 256, (240, 240, 4), dtype=np.uint8) for _ in range(2))
        rgba = r.render_pair(x4, y4, "0", "0", jpeg_views=(80, "standard"), **kw)
        assert all(v.dtype == np.uint8 and v.shape == (64, 64, 4) for v in rgba["perspective"].values())
        assert r.stats()["jpeg_device_images"] == 30
    finally:
        r.close()
