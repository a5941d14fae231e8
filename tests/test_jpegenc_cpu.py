"""JPG-SPEC v1 without a GPU: the header gs360/jpegenc.py builds and the NumPy restatement (tests/jpegenc_np.py) against Pillow and
against answers worked out by hand."""
import io

import numpy as np
import pytest

from gs360 import jpegenc

import jpegenc_cases as cases
import jpegenc_np as ref


def segments(data):
    """{marker: [payload, ...]} of a JFIF file's header segments, up to and including SOS"""
    out, p = {}, 2
    assert data[:2] == b"\xff\xd8"
    while True:
        assert data[p] == 0xFF
        marker, n = data[p + 1], int.from_bytes(data[p + 2:p + 4], "big")
        out.setdefault(marker, []).append(data[p + 4:p + 2 + n])
        p += 2 + n
        if marker == 0xDA:
            return out


def tables(payloads, dht):
    """{table id: bytes} of the DQT or DHT payloads of a file, however the writer grouped them into segments"""
    out = {}
    for pl in payloads:
        p = 0
        while p < len(pl):
            n = 1 + 16 + sum(pl[p + 1:p + 17]) if dht else 1 + 64
            assert pl[p] not in out
            out[pl[p]] = bytes(pl[p + 1:p + n])
            p += n
    return out


def pillow_file(a, quality, optimize=False):
    Image = pytest.importorskip("PIL.Image")
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", quality=quality, subsampling=0, optimize=optimize)
    return b.getvalue()


def decode(data):
    Image = pytest.importorskip("PIL.Image")
    return np.asarray(Image.open(io.BytesIO(data)))


def psnr(a, b):
    return 10.0 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


@pytest.mark.parametrize("quality", [100, 95, 75, 50, 10])
def test_header_quantiser_tables_equal_pillows(quality):
    rgb, gray = ref.noise_image(16, 16, 3), ref.noise_image(16, 16, 1)
    for a, C in ((rgb, 3), (gray, 1)):
        ours = segments(jpegenc.header(16, 16, C, quality, 8))
        theirs = segments(pillow_file(a, quality))
        assert tables(ours[0xDB], False) == tables(theirs[0xDB], False)
        assert sorted(tables(ours[0xDB], False)) == list(range(1 if C == 1 else 2))


def test_header_huffman_tables_equal_pillows_standard_ones():
    for a, C in ((ref.noise_image(16, 16, 3), 3), (ref.noise_image(16, 16, 1), 1)):
        ours = tables(segments(jpegenc.header(16, 16, C, 90, 8))[0xC4], True)
        theirs = tables(segments(pillow_file(a, 90, optimize=False))[0xC4], True)
        assert ours == theirs
        assert sorted(ours) == ([0x00, 0x10] if C == 1 else [0x00, 0x01, 0x10, 0x11])


def test_header_equals_the_restatements_and_names_its_parts():
    for C in (1, 3):
        for quality, restart in ((100, 8), (95, 1), (1, 65535)):
            h = jpegenc.header(37, 53, C, quality, restart)
            assert h == ref.header(37, 53, C, quality, restart)
            seg = segments(h)
            assert list(seg) == [0xE0, 0xDB, 0xC0, 0xC4, 0xDD, 0xDA]                   # APP0, DQT, SOF0, DHT, DRI, SOS
            assert seg[0xE0] == [b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"]      # JFIF 1.01, density 1:1, no thumbnail
            assert seg[0xDD] == [restart.to_bytes(2, "big")]
            sof = seg[0xC0][0]
            assert sof[0] == 8 and int.from_bytes(sof[1:3], "big") == 37 and int.from_bytes(sof[3:5], "big") == 53 and sof[5] == C
            assert all(sof[6 + 3 * c + 1] == 0x11 for c in range(C))                  # 4:4:4
    assert jpegenc.quality_for(None) == jpegenc.quality_for(1) == 100 and jpegenc.quality_for(2) == jpegenc.quality_for(31) == 95
    for bad in ((8, 8, 4, 90, 8), (8, 8, 3, 0, 8), (8, 8, 3, 101, 8), (8, 8, 3, 90, 0), (8, 8, 3, 90, 65536), (0, 8, 3, 90, 8), (8, 65536, 3, 90, 8)):
        with pytest.raises(ValueError):
            jpegenc.header(*bad)


def bits_of(data):
    return "".join(f"{b:08b}" for b in data)


@pytest.mark.parametrize("v", [0, 1, 127, 128, 129, 200, 255])
def test_a_flat_block_is_one_dc_code_and_eob(v):
    """a flat gray block of value v: every row product is 5793 * 8 * (v - 128) on u = 0 only, the DC (v - 128) * 8 up to the two
    roundings, every AC zero; at quality 100 (Q = 1) the scan is the DC difference's code, its bits, EOB (1010) and 1-padding"""
    a = np.full((8, 8), v, np.uint8)
    z = ref.coefficients(a, 100)
    assert z.shape == (1, 1, 1, 64) and not z[0, 0, 0, 1:].any()
    dc = int(z[0, 0, 0, 0])
    assert abs(dc - (v - 128) * 8) <= 1 and (v != 128 or dc == 0)
    size = abs(dc).bit_length()
    code, length = ref.huff_codes(ref.DC_LUMA)[size]
    want = f"{code:0{length}b}" + (f"{dc if dc >= 0 else dc + (1 << size) - 1:0{size}b}" if size else "") + "1010"
    want += "1" * (-len(want) % 8)
    scan = ref.scan(a, 100, 8)
    assert bits_of(scan.replace(b"\xff\x00", b"\xff")) == want


def test_an_interval_of_equal_blocks_is_ri_zero_difference_mcus():
    """16 x 32 flat RGB: 8 MCUs of three flat blocks.  In every interval the first MCU carries the three DC values, the others three zero
    differences (DC code of size 0) and three EOBs each; every interval restarts the prediction and ends on RSTm but the last"""
    a = np.full((16, 32, 3), (90, 160, 30), np.uint8)
    dc = [ref.huff_codes(ref.DC_LUMA), ref.huff_codes(ref.DC_CHROMA), ref.huff_codes(ref.DC_CHROMA)]
    eob = ["1010", "00", "00"]
    z = ref.coefficients(a, 100)[0, 0]

    def mcu(first):
        s = ""
        for c in range(3):
            v = int(z[c, 0]) if first else 0
            size = abs(v).bit_length()
            code, length = dc[c][size]
            s += f"{code:0{length}b}" + (f"{v if v >= 0 else v + (1 << size) - 1:0{size}b}" if size else "") + eob[c]
        return s
    for ri in (1, 4, 8, 3):
        want, n_int = b"", -(-8 // ri)
        for k in range(n_int):
            n = min(ri, 8 - k * ri)
            s = mcu(True) + mcu(False) * (n - 1)
            s += "1" * (-len(s) % 8)
            body = int(s, 2).to_bytes(len(s) // 8, "big").replace(b"\xff", b"\xff\x00")
            want += body + (bytes([0xFF, 0xD0 + k % 8]) if k + 1 < n_int else b"")
        assert ref.scan(a, 100, ri) == want, ri


@pytest.mark.parametrize("restart", [1, 4, 8])
def test_pillow_decodes_the_restatements_files(restart):
    for a in (ref.noise_image(), ref.photo_image(), ref.gray_of(ref.photo_image()), np.full((1, 1, 3), 9, np.uint8)):
        got = decode(ref.encode(a, 95, restart))
        assert got.shape == a.shape
        assert np.abs(got.astype(int) - a.astype(int)).mean() < 8.0


FIDELITY_INPUTS = {"noise 37x53x3": ref.noise_image, "photo 75x100x3": ref.photo_image, "gray 75x100": lambda: ref.gray_of(ref.photo_image())}


@pytest.mark.parametrize("quality", [100, 95])
@pytest.mark.parametrize("name", list(FIDELITY_INPUTS))
def test_fidelity_is_within_half_a_db_of_pillows_encoder(name, quality):
    """PSNR against the source of the decoded file: within 0.5 dB of Pillow's encode of the same array at the same quality and
    sampling.  Measured with Pillow 12.2 (ours - Pillow, quality 100 / 95): noise +0.39 / -0.03, photo +0.13 / -0.15,
    gray +0.16 / -0.19 dB."""
    a = FIDELITY_INPUTS[name]()
    ours = psnr(decode(ref.encode(a, quality, 8)), a)
    theirs = psnr(decode(pillow_file(a, quality)), a)
    print(f"{name} quality {quality}: ours {ours:.2f} dB, Pillow {theirs:.2f} dB, difference {ours - theirs:+.2f} dB")
    assert abs(ours - theirs) <= 0.5


def test_reciprocal_quantiser_is_exact():
    """the kernels divide by Q through floor(2^24 / Q) + 1: exact for every numerator the quantiser can see (and far beyond)"""
    n = np.arange(65536, dtype=np.uint64)
    for Q in range(1, 256):
        assert np.array_equal((n * np.uint64((1 << 24) // Q + 1)) >> np.uint64(24), n // np.uint64(Q)), Q


def test_the_device_tests_inputs_reach_the_cases_they_are_there_for():
    """tests/test_jpegenc_gpu.py compares these images' scans byte for byte: they must contain what the kernels can get wrong"""
    assert ref.scan(ref.noise_image(), 100, 8).count(b"\xff\x00") >= 40                   # stuffed bytes
    z = ref.coefficients(ref.photo_image(), 75)
    gaps = [np.diff(np.flatnonzero(np.r_[1, b[1:]])).max(initial=0) for b in z.reshape(-1, 64)]
    assert max(gaps) > 16                                                                 # a zero run over 15: ZRL
    assert np.abs(ref.coefficients(ref.checker_image(), 100)[..., 1:]).max() >= 512       # AC values of the largest size, 10 bits
    assert ref.scan(ref.noise_image(), 100, 1).count(b"\xff\xd7") >= 2                    # RST cycles past RST7


# ---- the alphabet inputs (tests/jpegenc_cases.py): the decoder pins the restatement, the counts pin the inputs -----------------------
GROUPS = cases.groups()
GROUP_IDS = [f"{g} q{q} Ri{ri}" for g, q, ri, _ in GROUPS]


@pytest.mark.parametrize("group", GROUPS, ids=GROUP_IDS)
def test_the_independent_decoder_returns_the_restatements_coefficients(group):
    """decode_scan builds its tables from the header's DHT and DRI bytes alone: the restatement's bit writer, Huffman codes, stuffing,
    padding and markers must give back the coefficients they were fed, on every input the device is compared on"""
    _g, quality, restart, images = group
    for name, a in images:
        H, W, C, n_mcu = cases.geometry(a)
        got = ref.decode_scan(ref.header(H, W, C, quality, restart), ref.scan(a, quality, restart), n_mcu, C)
        assert np.array_equal(got, ref.coefficients(a, quality).reshape(n_mcu, C, 64)), name


def test_the_independent_decoder_refuses_damaged_streams():
    a = ref.noise_image(16, 24, 3, seed=3)
    head, scan = ref.header(16, 24, 3, 100, 2), ref.scan(a, 100, 2)
    z = ref.coefficients(a, 100).reshape(6, 3, 64)
    assert np.array_equal(ref.decode_scan(head, scan, 6, 3), z)
    rst = scan.index(b"\xff\xd0")
    damaged = {"a wrong restart index": scan[:rst] + b"\xff\xd1" + scan[rst + 2:], "a lost byte": scan[:5] + scan[6:],
               "a lost marker": scan[:rst] + scan[rst + 2:], "a trailing byte": scan + b"\x00", "a truncated scan": scan[:-40],
               "an unstuffed 0xFF": scan.replace(b"\xff\x00", b"\xff", 1)}
    for what, data in damaged.items():
        try:
            same = np.array_equal(ref.decode_scan(head, data, 6, 3), z)
        except ValueError:
            continue
        assert not same, what
    # ... and first_difference names the place: the value bits of MCU 4's (interval 2's) first coefficient that is not +-1, inverted
    z2 = z.copy()
    m, c, i = next((m, c, i) for m in (4, 5) for c in range(3) for i in range(1, 64) if abs(z2[m, c, i]) > 1)
    z2[m, c, i] = -z2[m, c, i]
    other = ref.scan_from_coefficients(z2.reshape(2, 3, 3, 64), 2)
    said = ref.first_difference(head, other, scan, 6, 3)
    assert f"MCU {m} (interval 2), component {c}, zig-zag index {i}: {int(z2[m, c, i])} against {int(z[m, c, i])}" in said, said
    assert "does not decode" in ref.first_difference(head, scan[:-40], scan, 6, 3)


def test_pillow_decodes_the_alphabet_inputs():
    """every new image, at the first quality and restart interval it is used with (100 or 97): Pillow opens the restatement's file with
    the right shape and shows the picture, within the bound of test_pillow_decodes_the_restatements_files"""
    seen = set()
    for _g, quality, restart, images in GROUPS:
        for name, a in images:
            if name in seen:
                continue
            seen.add(name)
            got = decode(ref.encode(a, quality, restart))
            assert got.shape == a.shape, name
            assert np.abs(got.astype(int) - a.astype(int)).mean() < 8.0, name


# AC symbols the sweep cannot reach.  A single coefficient of size 10 needs an amplitude of at least 512 steps: at zig-zag positions
# 4 and 12 (runs 3 and 11 of the luma sweep) the rounded pixels give back 511, and in chroma the RGB gamut leaves no room for them
LUMA_AC_MISSING = {0x3A, 0xBA}
CHROMA_AC_MISSING = {0x0A, 0x3A, 0x7A, 0xAA, 0xBA, 0xEA, 0xFA}


def test_the_alphabet_inputs_reach_the_cases_they_are_there_for():
    """tests/test_jpegenc_alphabet_gpu.py compares the scans of these groups byte for byte; counted on the restatement's stream, they
    must hold what the entropy pass, the stuffing loop and the offsets kernel can get wrong"""
    reach = cases.Reach()
    for _g, quality, restart, images in GROUPS:
        for _name, a in images:
            reach.add(a, quality, restart)
    every = cases.all_symbols()
    assert len(every) == 162
    for t, missing in ((0, LUMA_AC_MISSING), (1, CHROMA_AC_MISSING)):
        assert every - reach.ac[t] == missing, (t, sorted(hex(s) for s in every - reach.ac[t]))
        assert {0x00, 0xF0} <= reach.ac[t]
        assert {(r << 4) | s for r in range(16) for s in range(1, 10)} <= reach.ac[t]        # every run at every size <= 9
    assert len(reach.ac[0]) == 160 and len(reach.ac[1]) == 155
    assert reach.zrl3 and reach.longest_word >= 56                                              # three ZRLs + code + value bits
    for t in (0, 1):
        assert {s for s, _ in reach.dc[t]} == set(range(12)), (t, sorted(reach.dc[t]))
        assert {(11, 1), (11, -1)} <= reach.dc[t]
    assert max(reach.block_bytes) == cases.FAT_BLOCK_WHOLE_BYTES >= 129                         # the stuffing loop's third pass
    assert any(65 <= n <= 128 for n in reach.block_bytes)                                       # ... and its second
    assert 63 in reach.ff_at and reach.ff_pad >= 1
    assert reach.carries == set(range(8))
    assert {256, 257} <= reach.n_int and max(reach.n_int) > 512
    print(f"luma AC {len(reach.ac[0])}/162, chroma AC {len(reach.ac[1])}/162, longest word {reach.longest_word} bits, largest block "
          f"{max(reach.block_bytes)} whole bytes, 0xFF at whole-byte indices {sorted(reach.ff_at)}, {reach.ff_pad} 0xFF pad bytes, "
          f"interval counts up to {max(reach.n_int)}")


def test_the_fat_block_is_what_the_search_found():
    a = cases.fat_block_image()
    z = ref.coefficients(a, 100)[0, :, 0, :]
    assert int(z[2, 0]) == -1024 and int(z[3, 0]) - int(z[2, 0]) >= 1024                      # a DC difference of size 11
    w = ref.BitWriter()
    ref.encode_block(w, [int(v) for v in z[3]], int(z[2, 0]), ref.huff_codes(ref.DC_LUMA), ref.huff_codes(ref.AC_LUMA))
    assert 8 * len(bytes(w.out).replace(b"\xff\x00", b"\xff")) + w.n == cases.FAT_BLOCK_BITS
    assert (7 + cases.FAT_BLOCK_BITS) // 8 == cases.FAT_BLOCK_WHOLE_BYTES
