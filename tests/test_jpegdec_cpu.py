"""JPD-SPEC v1 on the CPU: the NumPy restatement (tests/jpegdec_np.py) equals Pillow byte for byte on the matrix of DESIGN.md section
12, and gs360.jpegdec.parse() accepts those files with the right geometry, tables and segment offsets and refuses what the device path
does not take."""
import io

import numpy as np
import pytest

pytest.importorskip("PIL.Image")
from PIL import Image  # noqa: E402

from gs360 import capi, jpegdec  # noqa: E402

import jpegdec_cases as cases  # noqa: E402
import jpegdec_np as ref  # noqa: E402

MATRIX = cases.matrix_once()
assert len(MATRIX) == 228


@pytest.mark.parametrize("chunk", range(12))
def test_restatement_equals_pillow(chunk):
    for name, data in MATRIX[chunk::12]:
        assert np.array_equal(ref.decode(data), cases.pillow(data)), name


def test_parse_accepts_the_matrix():
    for name, data in MATRIX:
        d = jpegdec.parse(data)
        hd = ref.read_header(data)
        want = cases.pillow(data)
        assert (d.H, d.W) == want.shape[:2] and d.C == (1 if want.ndim == 2 else 3), name
        assert d.subsampling == (capi.JPEG_420 if "-s2-" in name else capi.JPEG_444), name
        assert d.restart == hd["restart"] == (3 if name.endswith("restart") else 0), name
        for c, (_i, _h, _v, tq) in enumerate(hd["comps"]):
            assert d.comp_tq[c] == tq and (d.comp_td[c], d.comp_ta[c]) == hd["sel"][c], name
            assert np.array_equal(d.quant[tq], hd["quant"][tq]), name
        for (cls, ident), (bits, vals) in hd["huff"].items():
            row = d.huff[2 * ident + cls]
            assert list(row[:16]) == bits and list(row[16:16 + len(vals)]) == vals and not row[16 + len(vals):].any(), name
        # the segments are the scan's bytes between its restart markers, in order, and the scan ends at EOI
        assert data[d.scan_off + d.scan_len:d.scan_off + d.scan_len + 2] == b"\xff\xd9", name
        assert data[d.scan_off:d.scan_off + d.scan_len] == hd["scan"], name
        segs = ref.split_segments(hd["scan"])
        assert d.segments.shape == (len(segs), 2) and len(segs) == (-(-d.n_mcu // d.restart) if d.restart else 1), name
        for (start, length), seg in zip(d.segments, segs):
            assert hd["scan"][start:start + length] == seg, name
        table, n_sub = jpegdec.segment_table(d)
        per = -(-d.segments[:, 1].astype(np.int64) // jpegdec.subseq_bytes())
        assert n_sub == per.sum() and list(table[:, 2]) == list(np.cumsum(per) - per), name
        assert list(table[:, 3]) == [k * d.restart for k in range(len(segs))], name


def _save(a, **kw):
    f = io.BytesIO()
    a.save(f, "JPEG", **kw)
    return f.getvalue()


def test_parse_refuses_what_the_device_does_not_take():
    rgb = Image.fromarray(cases.image(48, 80, "noise"))
    good = _save(rgb, quality=90)
    jpegdec.parse(good)
    refused = {
        "progressive": _save(rgb, quality=90, progressive=True),
        "4:2:2": _save(rgb, quality=90, subsampling=1),
        "CMYK": _save(rgb.convert("CMYK"), quality=90),
        "cut before EOI": good[:len(good) * 2 // 3],
        "EOI cut off": good[:-2],
        "not a JPEG": b"\x89PNG\r\n\x1a\n" + bytes(64),
    }
    for name, data in refused.items():
        with pytest.raises(jpegdec.Unsupported):
            jpegdec.parse(data)
    # every one of them still opens (or fails) on the host exactly as before: parse() never decides that
    assert np.asarray(Image.open(io.BytesIO(refused["progressive"]))).shape == (48, 80, 3)


def test_restatement_reports_corrupt_streams():
    data = cases.encode(cases.image(64, 64, "noise"), quality=90, subsampling=0)
    d = jpegdec.parse(data)
    cut = data[:d.scan_off + d.scan_len // 2] + b"\xff\xd9"
    with pytest.raises(ref.Corrupt):
        ref.decode(cut)
