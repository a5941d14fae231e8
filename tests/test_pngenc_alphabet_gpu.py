"""The device PNG encoder over RFC 1951's whole length and distance alphabets, on both sides of the 32 768 bound and at the largest sides
(the fixtures of tests/pngenc_cases.alphabet_cases(); tests/test_pngenc_cpu.py shows with the restatement alone that they reach what
they are built for): length, every stream byte, the guard behind the stream and every chunk's Adler pair, exactly."""
import zlib

import numpy as np
import pytest

from gs360 import capi, pngenc

import pngenc_cases as cases
import pngenc_np as ref
from test_pngenc_cpu import ALPHABET, decode_png, restated
from test_pngenc_gpu import check, run_deflate

pytestmark = pytest.mark.gpu


def run_and_check(ctx, names, **layout):
    check(names, run_deflate(ctx, [ALPHABET[n] for n in names], **layout), want=restated)


def test_every_match_length(ctx):
    run_and_check(ctx, ["lengths"])


def test_both_ends_of_every_distance_symbol_in_one_call(ctx):
    """52 jobs: four launch batches, jobs of two chunks in the first three, so the later batches' Adler pairs lie behind theirs"""
    names = list(cases.distance_cases())
    assert len(names) > 3 * capi.MAX_VIEWS
    run_and_check(ctx, names)


def test_the_distance_fixtures_from_padded_rows_and_an_offset_base_pointer(ctx):
    run_and_check(ctx, list(cases.distance_cases()), pad=10, offset=6)


def test_the_row_candidate_on_both_sides_of_32768(ctx):
    run_and_check(ctx, list(cases.bound_cases()))


@pytest.mark.parametrize("name", list(cases.side_cases()))
def test_the_largest_sides(ctx, name):
    """rows of 524 280 bytes across 8 chunks each; 65 535 rows of one byte"""
    run_and_check(ctx, [name])


def test_the_devices_files_inflate_and_decode_without_the_restatement(ctx):
    """whole files of encode_device: equal to the restatement's, and, on the device's bytes alone, inflated by zlib (which checks the
    block syntax and the Adler-32) to the filtered stream and decoded back to the input pixels"""
    names = ["lengths", "dist_32768", "side_wide_u16"]
    files = pngenc.encode_device(ctx, [ALPHABET[n] for n in names])
    for name, data in zip(names, files):
        img = ALPHABET[name]
        assert zlib.decompress(ref.idat_payload(data)) == ref.filtered_stream(img).tobytes(), name
        assert np.array_equal(decode_png(data, img), img), name
        assert data == restated(name)[2], name
