"""The device JPEG scans (gs360_jpeg_scan_u8, csrc/gs360_jpeg.hip) on the inputs of tests/jpegenc_cases.py: the whole Huffman alphabet
the standard tables can be driven to, words of three ZRLs, DC differences of size 11, a block of three stuffing passes, 0xFF on the
edge of a pass, images of more than 256 and 512 restart intervals behind other images, partial last intervals, an exact-fit capacity
and unaligned addresses.  Every scan is the restatement's (tests/jpegenc_np.py) byte for byte, on both slots; where one is not, both
streams go through the restatement's independent decoder and the failure names the first differing coefficient.
tests/test_jpegenc_cpu.py checks on the CPU that these inputs hold what they are here for."""
import numpy as np
import pytest

import gs360
from gs360 import jpegenc

import jpegenc_cases as cases
import jpegenc_np as ref
from test_jpegenc_gpu import GUARD, run_scans

pytestmark = pytest.mark.gpu

GROUPS = cases.groups()
GROUP_IDS = [f"{g} q{q} Ri{ri}" for g, q, ri, _ in GROUPS]
_WANT = {}


def want_scans(k):
    if k not in _WANT:
        _g, quality, restart, images = GROUPS[k]
        _WANT[k] = [ref.scan(a, quality, restart) for _n, a in images]
    return _WANT[k]


def assert_scan(what, a, quality, restart, n, data, want):
    """length, bytes and guard of one job; a mismatch is reported through the decoder"""
    if n != len(want) or data[:len(want)].tobytes() != want:
        if n == gs360.capi.JPEG_OVERFLOW:
            pytest.fail(f"{what}: JPEG_OVERFLOW reported for a scan of {len(want)} bytes")
        H, W, C, n_mcu = cases.geometry(a)
        got = data[:min(n, len(data))].tobytes()
        pytest.fail(f"{what}: " + ref.first_difference(ref.header(H, W, C, quality, restart), got, want, n_mcu, C))
    assert np.all(data[-GUARD:] == 0xA5), f"{what}: bytes written past the capacity"


@pytest.mark.parametrize("k", range(len(GROUPS)), ids=GROUP_IDS)
def test_every_group_matches_the_restatement_on_both_slots(ctx, k):
    group, quality, restart, images = GROUPS[k]
    wants = want_scans(k)
    for slot in (0, 1):
        got = run_scans(ctx, [a for _n, a in images], quality, restart, slot=slot)
        for (name, a), (n, data), want in zip(images, got, wants):
            assert_scan(f"{group} / {name}, quality {quality}, Ri {restart}, slot {slot}", a, quality, restart, n, data, want)


def test_exact_fit_and_one_byte_short_for_the_529_interval_image(ctx):
    """the last image of the placement call (its second launch batch, three trips of the offsets kernel's loop) with a capacity of
    exactly its scan, then one byte less: JPEG_OVERFLOW, nothing of it written, and every neighbour of the call as before"""
    k = GROUP_IDS.index("placement q100 Ri1")
    _g, quality, restart, images = GROUPS[k]
    wants = want_scans(k)
    at = [n for n, _a in images].index("184x184 rgb (529)")
    assert cases.geometry(images[at][1])[3] == 529
    for short in (0, 1):
        caps = [jpegenc.scan_bound(*cases.geometry(a)[:3], restart) for _n, a in images]
        caps[at] = len(wants[at]) - short
        got = run_scans(ctx, [a for _n, a in images], quality, restart, caps=caps, slot=short)
        for j, ((name, a), (n, data), want) in enumerate(zip(images, got, wants)):
            if short and j == at:
                assert n == gs360.capi.JPEG_OVERFLOW
                assert np.all(data == 0xA5), "an overflowing scan wrote into its buffer or its guard"
            else:
                assert_scan(f"{name} with the 529-interval image {short} bytes short", a, quality, restart, n, data, want)


class _Address:
    """an address inside a device allocation, as Context.jpeg_scan_dev reads a buffer: .ptr and .nbytes"""

    def __init__(self, buf, offset, nbytes):
        assert offset + nbytes <= buf.nbytes
        self.ptr, self.nbytes = buf.ptr + offset, nbytes


@pytest.mark.parametrize("quality", [100, cases.LOW_QUALITY])
def test_sources_and_outputs_at_unaligned_addresses(ctx, quality):
    """Context.jpeg_scan_dev passes on the addresses it is given, so a job can start anywhere in an allocation.  Sources begin 1, 2 and
    3 bytes past a dword inside a larger buffer (8 bytes of 0xEE before the image and 8 after it: the transform kernel loads whole
    dwords of a row), outputs at odd addresses; an RGB row of 100 pixels is 300 bytes, a gray one 100, so with a tight stride the
    rows of the odd-width crops below start on every byte alignment"""
    images = [a[:, :99] for _n, a in cases.restart_images()] + [cases.chunk_edge_image()[:, :251]]
    restart, bufs, jobs, outs = 7, [], [], []
    try:
        for j, a in enumerate(images):
            H, W, C, _ = cases.geometry(a)
            off = 8 + 1 + j % 3                                   # 9, 10, 11: one, two and three bytes past a dword
            host = np.full(off + a.size + 8, 0xEE, np.uint8)
            host[off:off + a.size] = a.reshape(-1)
            src = ctx.to_device(host)
            cap = jpegenc.scan_bound(H, W, C, restart)
            out = ctx.alloc(16 + cap + GUARD)
            ctx.memset(out, 0xA5)
            bufs += [src, out]
            lead = 1 + 2 * j                                      # 1, 3, 5
            outs.append((out, lead, cap))
            jobs.append((_Address(src, off, a.size), H, W, C, 0, _Address(out, lead, cap), cap))
        d_len = ctx.alloc(8 * len(jobs))
        bufs.append(d_len)
        ctx.jpeg_scan_dev(jobs, d_len, quality=quality, restart=restart)
        lengths = ctx.download(d_len, (len(jobs),), np.uint64)
        for a, n, (out, lead, cap) in zip(images, lengths, outs):
            whole = ctx.download(out, (out.nbytes,), np.uint8)
            assert np.all(whole[:lead] == 0xA5), "bytes written in front of the output address"
            assert_scan(f"source {a.shape} at an unaligned address, output at +{lead}", a, quality, restart, int(n),
                        whole[lead:lead + cap + GUARD], ref.scan(a, quality, restart))
    finally:
        for b in bufs:
            ctx.free(b)
