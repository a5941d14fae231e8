"""Input colour stage on the layouts the stage's own tests never reach: padded and odd strides, a separate destination, the
partial groups at a row's end and the quantiser variants of the per-pixel kernels.

Calls go through Context.color_apply_dev / color_apply16_dev so that dst and both strides are the test's own.  Expected values
are the NumPy oracle's (oracle.color_np.color_pipeline).  Every case asserts the image rows exactly and, with a separate dst,
that every byte of a sentinel-filled dst outside the W*C samples of each row -- row padding and a guard area behind the last
row -- is unchanged.

Which kernel a layout selects (gs360_color.hip): pointers and strides that are all multiples of 4 take the dword kernels (four
8-bit pixels or two 16-bit pixels per thread, with a per-pixel tail for the last partial group of a row), anything else the
one-pixel-per-thread kernels.  With tight rows a 3-channel row is dword-aligned only for W % 4 == 0 (8-bit) or even W (16-bit),
so the 3-channel tails are reached by the padded layouts alone, and the 4-channel one-pixel kernels by the odd strides alone.
"""
import functools

import numpy as np
import pytest

from conftest import ROOT
from gs360 import color
from oracle import color_np

pytestmark = pytest.mark.gpu

G = np.load(ROOT / "tests" / "golden" / "color_goldens.npz")
TABLE, DMIN, DMAX = G["lut_dom9_table"], G["lut_dom9_dmin"], G["lut_dom9_dmax"]
GUARD = 64                     # bytes behind the last row that must stay untouched
SRC_FILL, DST_FILL = 0x5A, 0xA5


def stride_of(layout, row_bytes, sample_bytes):
    """byte stride of a layout.  `padded`: the next multiple of 4 plus 8 (dword kernels); `odd`: a stride that is no multiple of 4
    -- the first odd number above the row for 8-bit samples (W*C + 1 is itself a multiple of 4 for the 3-channel rows of W = 1029
    and W = 5), stride % 4 == 2 for 16-bit samples, whose strides must be even."""
    if layout == "tight":
        return row_bytes
    padded = (row_bytes + 3) // 4 * 4 + 8
    if layout == "padded":
        assert padded % 4 == 0
        return padded
    odd = ((row_bytes + 1) | 1) if sample_bytes == 1 else padded + 2
    assert odd % 4 != 0 and odd % sample_bytes == 0 and odd > row_bytes
    return odd


def run_layout(ctx, apply, plan, image, want, layout, separate, red):
    """one call on `image` (H x W x C, uint8 or uint16) laid out with `layout`; in place or into a sentinel-filled dst"""
    H, W, Cn = image.shape
    row = W * Cn * image.itemsize
    stride = stride_of(layout, row, image.itemsize)
    total = H * stride + GUARD
    inside = np.zeros(total, bool)
    inside[:H * stride].reshape(H, stride)[:, :row] = True
    src_host = np.full(total, SRC_FILL, np.uint8)
    src_host[inside] = np.ascontiguousarray(image).view(np.uint8).reshape(-1)
    d_src = ctx.to_device(src_host)
    d_dst = ctx.to_device(np.full(total, DST_FILL, np.uint8)) if separate else None
    before = np.full(total, DST_FILL, np.uint8) if separate else src_host
    arg = 0 if layout == "tight" else stride              # 0 = tight rows, the library's default
    try:
        apply(plan, d_src, H, W, Cn, dst=d_dst, red_index=red, src_stride=arg, dst_stride=arg)
        got = ctx.download(d_dst if separate else d_src, (total,))
        if separate:
            assert np.array_equal(ctx.download(d_src, (total,)), src_host), "the source was written"
    finally:
        ctx.free(d_src)
        if separate:
            ctx.free(d_dst)
    assert np.array_equal(got[inside], np.ascontiguousarray(want).view(np.uint8).reshape(-1)), "image rows differ from the oracle"
    assert np.array_equal(got[~inside], before[~inside]), "bytes outside the image rows were written"


# ---- 8-bit: cube and per-pixel plans ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plans8(ctx):
    """one plan with the 2^24 cube and one that evaluates per pixel (option color_cube = 0 around its creation)"""
    lut = color.CubeLUT(TABLE.shape[0], TABLE, DMIN, DMAX)
    pos, thr = color.level_positions(lut), color.output_thresholds("srgb")
    plans = {"cube": ctx.color_plan(TABLE, pos, thr)}
    with ctx.options(color_cube=0):
        plans["pixel"] = ctx.color_plan(TABLE, pos, thr)
    yield plans
    for p in plans.values():
        ctx.color_plan_free(p)


@functools.lru_cache(maxsize=None)
def image8(H, W, Cn):
    img = np.random.default_rng(1000 * H + 10 * W + Cn).integers(0, 256, (H, W, Cn), dtype=np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def want8(H, W, Cn, red):
    return color_np.color_pipeline(image8(H, W, Cn), TABLE, DMIN, DMAX, "srgb", red_index=red)


# (3, 1029): cube quad kernel -- thread 0's second group is full, thread 1's second group holds one pixel; LUT quad kernel -- second
#            segment, one full group and a one-pixel tail
# (2051, 5): 2051 one-segment rows over the 2048 persistent blocks of the LUT quad kernel: three blocks take the prefetched second
#            iteration; each row is a full group plus a one-pixel tail (non-tight layouts only)
# (2, 3):    nothing but a tail
SHAPES8 = [(3, 1029, "tight"), (3, 1029, "padded"), (3, 1029, "odd"), (2051, 5, "padded"), (2051, 5, "odd"),
           (2, 3, "tight"), (2, 3, "padded"), (2, 3, "odd")]


@pytest.mark.parametrize("Cn", [3, 4])
@pytest.mark.parametrize("kind", ["cube", "pixel"])
@pytest.mark.parametrize("H,W,layout", SHAPES8)
def test_u8_layouts(ctx, plans8, H, W, layout, kind, Cn):
    for red in (0, 2):
        for separate in (False, True):
            run_layout(ctx, ctx.color_apply_dev, plans8[kind], image8(H, W, Cn), want8(H, W, Cn, red), layout, separate, red)


# ---- 16-bit ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plans16(ctx):
    """the 16-bit quantiser pieces take about a second to build on the host: once per space"""
    plans = {space: ctx.color_plan16(TABLE, DMIN, DMAX, *color.output_pieces16(space)) for space in ("srgb", "passthrough")}
    yield plans
    for p in plans.values():
        ctx.color_plan16_free(p)


@functools.lru_cache(maxsize=None)
def image16(H, W, Cn):
    img = np.random.default_rng(1000 * H + 10 * W + Cn + 7).integers(0, 65536, (H, W, Cn), dtype=np.uint16)
    img[0, :, 0] = np.linspace(0, 65535, W).astype(np.uint16)            # sweeps every piece of the quantiser
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def want16(H, W, Cn, red, space):
    return color_np.color_pipeline(image16(H, W, Cn), TABLE, DMIN, DMAX, space, red_index=red)


# (3, 515): two blocks of the pair kernel plus the odd-width tail; (2, 1): the tail alone.  `odd` here is stride % 4 == 2, which
# selects the one-pixel kernel (as does the tight 3-channel row of an odd width)
@pytest.mark.parametrize("layout", ["tight", "padded", "odd"])
@pytest.mark.parametrize("Cn", [3, 4])
@pytest.mark.parametrize("space", ["srgb", "passthrough"])
@pytest.mark.parametrize("H,W", [(3, 515), (2, 1)])
def test_u16_layouts(ctx, plans16, H, W, space, Cn, layout):
    stride = stride_of(layout, W * Cn * 2, 2)
    assert stride % 2 == 0 and (layout != "padded" or stride % 4 == 0) and (layout != "odd" or stride % 4 == 2)
    for red in (0, 2):
        for separate in (False, True):
            run_layout(ctx, ctx.color_apply16_dev, plans16[space], image16(H, W, Cn), want16(H, W, Cn, red, space), layout, separate, red)


# ---- the per-pixel kernels' quantiser variants ------------------------------------------------------------------------------------
def fixups_of(thr):
    """what the library's color_build_bins decides from thr[1..255]: 1 or 2 in-bin compares after the 1024-bin table, or 0 (binary
    search) when some bin holds more than two thresholds"""
    t = thr[1:].astype(np.float32)
    edges = (np.arange(1025, dtype=np.float32) / np.float32(1024.0)).astype(np.float32)
    worst = 0
    for i in range(1024):
        above = t[t > edges[i]]
        inside = np.count_nonzero(above <= np.float32(1.0)) if i == 1023 else np.count_nonzero(above < edges[i + 1])
        worst = max(worst, inside)
    return 1 if worst <= 1 else (2 if worst == 2 else 0)


QUANTISERS = [("one_per_bin", lambda k: k / 520.0, 1), ("two_per_bin", lambda k: 0.3 + k / 1800.0, 2), ("dense", lambda k: 0.5 + k * 1e-5, 0),
              ("ties_and_never", lambda k: np.where(k < 200, (k // 4) / 64.0, np.inf), 1), ("zero_start", lambda k: np.maximum(k - 3, 0) / 300.0, 1)]


assert {f for _, _, f in QUANTISERS} == {0, 1, 2}          # a 1-compare, a 2-compare and a binary-search plan


@pytest.mark.parametrize("Cn", [3, 4])
@pytest.mark.parametrize("name,thr_of_k,fixups", QUANTISERS)
def test_per_pixel_quantiser_variants(ctx, name, thr_of_k, fixups, Cn):
    """1-compare, 2-compare and binary-search plans without the cube: 33 x 64 takes the dword kernel, 33 x 63 the byte kernel
    (3 channels) or the dword kernel's three-pixel tail (4 channels)"""
    table, dmin, dmax = G["lut_id2_table"], G["lut_id2_dmin"], G["lut_id2_dmax"]      # identity cube: LUT output = level / 255
    pos = color.level_positions(color.CubeLUT(2, table, dmin, dmax))
    thr = np.empty(256, np.float32)
    thr[0] = -np.inf
    thr[1:] = thr_of_k(np.arange(1, 256))
    assert fixups_of(thr) == fixups, name
    with ctx.options(color_cube=0):
        plan = ctx.color_plan(table, pos, thr)
    try:
        for W in (64, 63):
            img = np.random.default_rng(2 + W + Cn).integers(0, 256, (33, W, Cn), dtype=np.uint8)
            img[0, :, 0] = np.arange(W) * 4
            img[1, :, 1] = 255 - np.arange(W)
            x = color_np.trilinear(img[..., :3].astype(np.float32) / np.float32(255.0), table, dmin, dmax)
            want = img.copy()
            want[..., :3] = np.searchsorted(thr[1:], np.clip(x, 0, 1), side="right").astype(np.uint8)
            run_layout(ctx, ctx.color_apply_dev, plan, img, want, "tight", False, 0)
    finally:
        ctx.color_plan_free(plan)
