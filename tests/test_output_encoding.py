"""The definition the output encoders of the pass are pinned to, checked on the CPU.

sRGB8: the reference stores to_unorm8(convert_linear_to_srgb(v)) (srgb_utility.glsl:20-34, shading_pass.frag.glsl:888-892):
a float pow, then v * 255 + 0.5 truncated.  The oracle restates it (oracle_shading.c) and scans every float of [0, 1]
for the first float of each code (oracle.srgb8_code_starts); the kernels count those starts
(tests/test_gpu_output_encoding.py checks every float of [0, 1] on the GPU).  Half split: packHalf2x16 semantics."""
import numpy as np
import pytest

import oracle
from helpers import NAN_BITS, FLOAT_MAX_BITS, encoder_specials, from_bits, half_sweep_chunks, half_test_values, unorm8
from oracle import reference


@pytest.fixture(scope="module")
def starts():
    status, starts = oracle.srgb8_code_starts()
    assert status == 0, "the oracle's sRGB8 code decreases somewhere in [0, 1] or skips a code (status %d)" % status
    return starts


def pixels(values, channel):
    """one value per pixel in `channel`, 0.5 in the others"""
    rgba = np.full((len(values), 4), 0.5, np.float32)
    rgba[:, channel] = values
    return rgba


def test_code_table_is_monotone_and_complete(starts):
    assert starts[0] == 0
    assert (np.diff(starts.astype(np.int64)) > 0).all()
    assert starts[255] < 0x3F800000
    # each start is the first float of its code: the float below has the code before
    for channel in range(3):
        at = oracle.encode_srgb8(pixels(from_bits(starts[1:]), channel))[:, channel]
        below = oracle.encode_srgb8(pixels(from_bits(starts[1:] - 1), channel))[:, channel]
        assert np.array_equal(at, np.arange(1, 256)), channel
        assert np.array_equal(below, np.arange(0, 255)), channel


def test_code_table_against_float64(starts):
    """The exact threshold of code c is srgb_to_linear((c - 0.5) / 255), here in float64 and rounded up to the first
    float at or above it.  The float arithmetic of the reference moves 171 of the 255 boundaries, by 1 to 4 floats and
    in both directions, 219 floats in all (0x1.3e4566p-13 is code 1, not 0: the rounding of v * 255 + 0.5 alone moves
    the first boundary).  A wrong constant or branch would move them much further."""
    c = np.arange(1, 256)
    x = (c - 0.5) / 255.0
    exact = np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)
    first = exact.astype(np.float32)
    first = np.where(first.astype(np.float64) < exact, np.nextafter(first, np.float32(1)), first)
    moved = starts[1:].astype(np.int64) - first.view(np.uint32).astype(np.int64)
    assert np.abs(moved).max() <= 4, moved
    assert (moved != 0).sum() == 171 and np.abs(moved).sum() == 219, ((moved != 0).sum(), np.abs(moved).sum())


@pytest.mark.skipif(not reference.available(), reason="oracle/_ref has not been built")
def test_code_table_against_the_reference_shader(starts):
    """convert_linear_to_srgb of the reference's srgb_utility.glsl compiled as C++, stored as UNORM8: code c at each
    start, c - 1 at the float below"""
    import ctypes as C
    L = reference.shader(reference.variants()[0])
    value, back = C.c_float(), C.c_float()
    for code in range(1, 256):
        for bits, expected in ((int(starts[code]), code), (int(starts[code]) - 1, code - 1)):
            L.ref_srgb(C.c_float(from_bits([bits])[0]), C.byref(value), C.byref(back))
            got = int(unorm8([value.value])[0])
            assert got == expected, "reference: %s -> code %d, the oracle's table says %d" % (float(from_bits([bits])[0]).hex(), got, expected)


def test_srgb8_specials():
    """signed zeros and everything below 0 -> 0, everything above 1 -> 255, NaN -> 0, in RGB and in alpha"""
    special = {"zeros": (from_bits([0, 0x80000000]), 0),
               "negatives": (from_bits([0x80000001, 0x807FFFFF, 0xB3800000, 0xBF000000, 0xBF800000, 0xFF7FFFFF]), 0),
               "-inf": (from_bits([0xFF800000]), 0),
               "above one": (from_bits([0x3F800001, 0x3FC00000, 0x40000000, 0x4B000000, 0x7149F2CA, FLOAT_MAX_BITS]), 255),
               "+inf": (from_bits([0x7F800000]), 255),
               "NaN": (from_bits(NAN_BITS), 0)}
    for name, (values, code) in special.items():
        for channel in range(4):
            got = oracle.encode_srgb8(pixels(values, channel))[:, channel]
            assert (got == code).all(), (name, channel, got)
    # and the general rule on the rest of the specials: sRGB code of the value clamped to [0, 1], alpha its UNORM8
    values = encoder_specials()
    got = oracle.encode_srgb8(np.repeat(values[:, None], 4, axis=1))
    assert np.array_equal(got[:, 3], unorm8(values))
    clamped = np.where(np.isnan(values), np.float32(0), np.clip(values, np.float32(0), np.float32(1))).astype(np.float32)
    assert np.array_equal(got[:, :3], oracle.encode_srgb8(np.repeat(clamped[:, None], 4, axis=1))[:, :3])


def split_halves(values, output_linear_rgb):
    """values -> (half bits reassembled from the bytes of frame_bits 2 and 1, the bytes)"""
    rgba = np.zeros((-(-len(values) // 3), 4), np.float32)
    rgba[:, :3] = np.append(values, np.zeros(-len(values) % 3, np.float32)).reshape(-1, 3)
    low = oracle.encode_half_bits(rgba, 1, output_linear_rgb)
    high = oracle.encode_half_bits(rgba, 2, output_linear_rgb)
    assert (low[:, 3] == 255).all() and (high[:, 3] == 255).all()
    halves = (high[:, :3].astype(np.uint16) << 8) | low[:, :3].astype(np.uint16)
    return halves.reshape(-1)[:len(values)], low, high


def check_halves(values, halves):
    nan = np.isnan(values)
    with np.errstate(over="ignore"):
        expected = values[~nan].astype(np.float16).view(np.uint16)
    wrong = np.flatnonzero(halves[~nan] != expected)
    assert wrong.size == 0, "%d floats split into the wrong half, e.g. %s" % (wrong.size, [
        (float(values[~nan][i]).hex(), hex(int(halves[~nan][i])), hex(int(expected[i]))) for i in wrong[:8]])
    # NaN: a NaN half with the sign of the input
    h = halves[nan]
    assert ((h & 0x7C00) == 0x7C00).all() and ((h & 0x03FF) != 0).all(), [hex(int(v)) for v in h]
    assert np.array_equal(h >> 15, (values[nan].view(np.uint32) >> 31).astype(np.uint16))


@pytest.mark.parametrize("output_linear_rgb", [False, True])
def test_half_split_against_numpy(output_linear_rgb):
    values = half_test_values()
    halves, low, high = split_halves(values, output_linear_rgb)
    check_halves(values, halves)
    # every byte value occurs in both bytes (the round trip of output_linear_rgb keeps all 256 of them), except the high
    # bytes of NaN halves with a payload other than the quiet bit: the split's NaN is sign | 0x7E00
    assert np.array_equal(np.unique(low[:, :3]), np.arange(256))
    assert np.array_equal(np.unique(high[:, :3]), np.setdiff1d(np.arange(256), [0x7D, 0x7F, 0xFD, 0xFF]))


def test_half_split_sweeps():
    """every float of the half subnormal range and of the overflow range"""
    for values in half_sweep_chunks():
        halves, _, _ = split_halves(values, False)
        check_halves(values, halves)
