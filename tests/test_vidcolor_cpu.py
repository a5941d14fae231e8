"""VID-COLOR v1 without a GPU: the NumPy restatement (tests/vidcolor_np.py) against a float64 evaluation of the mathematics the spec
restates, written here and shared with nothing; the bounds are conditions of the formats (half a level of rounding plus half a level
of everything else at 8 bits, one input step = 64 of 65535 at 10 bits).  And the Y4M reader on what it accepts and refuses."""
import io

import numpy as np
import pytest

import vidcolor_np as ref
from gs360 import vidcolor, y4m

KR, KB = 0.2126, 0.0722


def _xyz(chroma):
    cols = np.array([[x / y, 1.0, (1 - x - y) / y] for x, y in chroma[:3]]).T
    wx, wy = chroma[3]
    white = np.array([wx / wy, 1.0, (1 - wx - wy) / wy])
    return cols @ np.diag(np.linalg.inv(cols) @ white)


M_IDEAL = np.linalg.inv(_xyz([(.630, .340), (.310, .595), (.155, .070), (.3127, .3290)])) @ \
    _xyz([(.640, .330), (.300, .600), (.150, .060), (.3127, .3290)])


def ideal_linear(Y, U, V, depth, full_range):
    """float64: samples -> linear SMPTE-C RGB in [0,1], (3, n)"""
    s, top = 2.0 ** (depth - 8), 2.0 ** depth - 1
    Y, U, V = (np.minimum(np.asarray(a, np.float64), top) for a in (Y, U, V))
    if full_range:
        y, cb, cr = Y / top, (U - 128 * s) / top, (V - 128 * s) / top
    else:
        y, cb, cr = (Y - 16 * s) / (219 * s), (U - 128 * s) / (224 * s), (V - 128 * s) / (224 * s)
    r = y + 2 * (1 - KR) * cr
    b = y + 2 * (1 - KB) * cb
    g = (y - KR * r - KB * b) / (1 - KR - KB)
    v = np.clip(np.stack([r, g, b]), 0.0, 1.0)
    lin = np.where(v < 0.081, v / 4.5, ((v + 0.099) / 1.099) ** (1 / 0.45))
    return np.clip(M_IDEAL @ lin, 0.0, 1.0)


def ideal_encode(l, keep_rec709, outmax):
    if keep_rec709:
        e = np.where(l < 0.018, 4.5 * l, 1.099 * l ** 0.45 - 0.099)
    else:
        e = np.where(l <= 0.0031308, 12.92 * l, 1.055 * l ** (1 / 2.4) - 0.055)
    return e.T * outmax            # (n, 3), unrounded


def worst(Y, U, V, depth, full_range):
    """largest |restatement - unrounded ideal| over the triples, for (sRGB, Rec.709)"""
    l = ideal_linear(Y, U, V, depth, full_range)
    outmax = 255 if depth == 8 else 65535
    q = ref.rgb14(Y, U, V, depth, full_range)
    return [float(np.abs(ref.levels(q, depth, keep).astype(np.float64) - ideal_encode(l, keep, outmax)).max()) for keep in (False, True)]


def test_every_8_bit_triple_is_within_one_level_of_the_ideal():
    v = np.arange(256)
    U, V = (a.ravel() for a in np.meshgrid(v, v, indexing="ij"))
    err = np.zeros(2)
    for y in range(0, 256, 8):
        Y = np.repeat(np.arange(y, y + 8), U.size)
        err = np.maximum(err, worst(Y, np.tile(U, 8), np.tile(V, 8), 8, False))
    print("8-bit limited, worst error in levels (sRGB, Rec.709):", err)
    assert err[0] <= 1.0 and err[1] <= 1.0


def extremes10():
    """every 10-bit triple with two components at 0 or 1023"""
    out = []
    for free in range(3):
        for a in (0, 1023):
            for b in (0, 1023):
                t = np.empty((1024, 3), np.int64)
                t[:, free] = np.arange(1024)
                t[:, [c for c in range(3) if c != free]] = (a, b)
                out.append(t)
    return np.concatenate(out)


def test_10_bit_triples_are_within_one_input_step_of_the_ideal():
    rng = np.random.default_rng(1710)
    t = np.concatenate([rng.integers(0, 1024, size=(4_000_000, 3)), extremes10()])
    err = worst(t[:, 0], t[:, 1], t[:, 2], 10, False)
    print("10-bit limited, worst error of 65535 (sRGB, Rec.709):", err)
    assert err[0] <= 64.0 and err[1] <= 64.0


def test_full_range_at_both_depths():
    rng = np.random.default_rng(1711)
    t = rng.integers(0, 256, size=(1_000_000, 3))
    err8 = worst(t[:, 0], t[:, 1], t[:, 2], 8, True)
    t = np.concatenate([rng.integers(0, 1024, size=(1_000_000, 3)), extremes10()])
    err10 = worst(t[:, 0], t[:, 1], t[:, 2], 10, True)
    print("full range, worst error (8-bit levels, 10-bit of 65535):", err8, err10)
    assert max(err8) <= 1.0 and max(err10) <= 64.0
    # full-range white and black are the ends of the output
    assert ref.convert_triples([255, 0], [128, 128], [128, 128], 8, True).tolist() == [[255] * 3, [0] * 3]
    assert ref.convert_triples([1023, 0], [512, 512], [512, 512], 10, True).tolist() == [[65535] * 3, [0] * 3]
    assert ref.convert_triples([235, 16], [128, 128], [128, 128], 8, False).tolist() == [[255] * 3, [0] * 3]


def test_samples_above_1023_are_clamped():
    rng = np.random.default_rng(1712)
    t = rng.integers(0, 1024, size=(4096, 3))
    big = t.copy()
    big[t >= 1000] = rng.integers(1024, 65536, size=int((t >= 1000).sum()))
    clamped = np.minimum(big, 1023)
    assert (big > 1023).sum() > 100
    for full in (False, True):
        assert np.array_equal(ref.convert_triples(big[:, 0], big[:, 1], big[:, 2], 10, full),
                              ref.convert_triples(clamped[:, 0], clamped[:, 1], clamped[:, 2], 10, full))


def test_the_primaries_matrix():
    m = vidcolor.primaries_matrix()
    assert np.abs(m.sum(axis=1) - 1.0).max() <= 1e-12          # white stays white
    assert np.abs(m - M_IDEAL).max() <= 1e-12
    want = [[1.06537903, -0.05540087, -0.00997816], [-0.01963255, 1.03636309, -0.01673054], [0.00163205, 0.00441237, 0.99395558]]
    assert np.abs(m - np.array(want)).max() < 5e-9


def test_the_tables():
    lin = vidcolor.linear_table()
    assert lin.shape == (16384,) and lin.dtype == np.float32 and lin[0] == 0.0 and lin[-1] == 1.0
    # rising, but for the Rec.709 constants' own step down at v = 0.081 (0.018 on the toe, 0.017948 on the power segment)
    assert np.flatnonzero(np.diff(lin) <= 0).tolist() == [int(np.ceil(0.081 * 16383)) - 1]
    for keep in (False, True):
        for outmax in (255, 65535):
            enc = vidcolor.encode_table(keep, outmax)
            assert enc.shape == (1024, 2) and enc[0, 0] == 0.0 and enc[-1, 0] + enc[-1, 1] == outmax and np.all(enc[:, 1] > 0)
    with pytest.raises(ValueError):
        vidcolor.VideoColor(12)


def test_chroma_is_replicated():
    rng = np.random.default_rng(1713)
    H, W = 5, 7
    y = rng.integers(16, 236, size=(H, W), dtype=np.uint8)
    for sub in ("420", "422", "444"):
        ch, cw = ref.chroma_shape(H, W, sub)
        u, v = (rng.integers(16, 241, size=(ch, cw), dtype=np.uint8) for _ in range(2))
        got = ref.convert(y, u, v, 8, sub)
        sx, sy = ref.SUBS[sub]
        for yy in range(H):
            for xx in range(W):
                one = ref.convert_triples([y[yy, xx]], [u[yy >> sy, xx >> sx]], [v[yy >> sy, xx >> sx]], 8)[0]
                assert np.array_equal(got[yy, xx], one)


# ---- the Y4M reader ----------------------------------------------------------------------------------------------------------------
def stream_of(tag, W, H, frames, extra=""):
    sub, depth = y4m.COLORSPACES[tag]
    ch, cw = ref.chroma_shape(H, W, sub)
    head = "YUV4MPEG2 W{} H{} F30:1 Ip A1:1 C{}{}\n".format(W, H, tag, extra).encode()
    body = b""
    for planes in frames:
        assert [p.shape for p in planes] == [(H, W), (ch, cw), (ch, cw)]
        body += b"FRAME\n" + b"".join(p.astype("<u2" if depth == 10 else np.uint8).tobytes() for p in planes)
    return head + body


def random_frames(rng, tag, W, H, n):
    sub, depth = y4m.COLORSPACES[tag]
    ch, cw = ref.chroma_shape(H, W, sub)
    return [tuple(rng.integers(0, 1 << depth, size=s) for s in ((H, W), (ch, cw), (ch, cw))) for _ in range(n)]


@pytest.mark.parametrize("tag", sorted(y4m.COLORSPACES))
def test_y4m_reads_every_accepted_tag_at_odd_sizes(tag):
    rng = np.random.default_rng(len(tag))
    for W, H in ((7, 5), (1, 1), (8, 2)):
        frames = random_frames(rng, tag, W, H, 3)
        reader = y4m.Y4MReader(io.BytesIO(stream_of(tag, W, H, frames, " XCOLORRANGE=FULL" if W == 7 else "")))
        h = reader.header
        assert (h.width, h.height, (h.subsampling, h.depth), h.full_range, h.colorspace) == (W, H, y4m.COLORSPACES[tag], W == 7, tag)
        got = list(reader)
        assert len(got) == 3 and reader.frames_read == 3
        for g, w in zip(got, frames):
            assert all(a.dtype.itemsize == (2 if h.depth == 10 else 1) and np.array_equal(a, b) for a, b in zip(g, w))


def test_y4m_defaults_and_frame_parameters():
    frames = random_frames(np.random.default_rng(5), "420jpeg", 6, 4, 1)
    data = stream_of("420jpeg", 6, 4, frames).replace(b" C420jpeg", b"").replace(b"FRAME\n", b"FRAME Ip\n")
    reader = y4m.Y4MReader(io.BytesIO(data))
    assert (reader.header.subsampling, reader.header.depth, reader.header.full_range) == ("420", 8, False)
    assert np.array_equal(next(iter(reader))[0], frames[0][0])


@pytest.mark.parametrize("what, data", [
    ("mono", b"YUV4MPEG2 W4 H4 F30:1 Ip Cmono\n"),
    ("12 bits", b"YUV4MPEG2 W4 H4 F30:1 Ip C420p12\n"),
    ("16 bits", b"YUV4MPEG2 W4 H4 F30:1 Ip C444p16\n"),
    ("top field first", b"YUV4MPEG2 W4 H4 F30:1 It C420jpeg\n"),
    ("bottom field first", b"YUV4MPEG2 W4 H4 F30:1 Ib C420jpeg\n"),
    ("no size", b"YUV4MPEG2 F30:1 Ip C420jpeg\n"),
    ("not y4m", b"P6\n4 4\n255\n"),
    ("empty", b""),
    ("range", b"YUV4MPEG2 W4 H4 C420jpeg XCOLORRANGE=WIDE\n"),
])
def test_y4m_refuses(what, data):
    with pytest.raises(y4m.Y4MError):
        y4m.Y4MReader(io.BytesIO(data))


def test_y4m_refuses_a_truncated_frame_and_a_stray_marker():
    frames = random_frames(np.random.default_rng(6), "422p10", 5, 3, 2)
    data = stream_of("422p10", 5, 3, frames)
    reader = y4m.Y4MReader(io.BytesIO(data[:-3]))
    it = iter(reader)
    next(it)
    with pytest.raises(y4m.Y4MError, match="truncated"):
        next(it)
    with pytest.raises(y4m.Y4MError, match="FRAME"):
        list(y4m.Y4MReader(io.BytesIO(data.replace(b"FRAME\n", b"FRANE\n"))))
