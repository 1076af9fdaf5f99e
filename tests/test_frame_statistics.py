"""The numpy restatement of the frame statistics (vulkan_renderer_amd/frame_statistics.py) against exact rational
arithmetic, and the host side of their C-ABI (include/vkr_frame_statistics.h).  The GPU tests
(tests/test_gpu_frame_statistics.py) pin the kernels against the restatement bit for bit."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from vulkan_renderer_amd import capi
from vulkan_renderer_amd import frame_statistics as fs


def bits(values):
    return np.asarray(values, np.float64).view(np.uint64)


def exact_add(a, b):
    """a + b in binary64 from first principles: the rational sum rounded once (float() of a Fraction rounds to
    nearest even), and the IEEE rules for what is not a rational number"""
    a, b = float(a), float(b)
    if math.isnan(a) or math.isnan(b) or (math.isinf(a) and math.isinf(b) and a != b):
        return math.nan
    if math.isinf(a) or math.isinf(b):
        return a if math.isinf(a) else b
    total = Fraction(a) + Fraction(b)
    if total == 0:
        # an exact zero sum is +0 (round to nearest) unless both terms are -0
        return -0.0 if (math.copysign(1.0, a) < 0 and math.copysign(1.0, b) < 0) else 0.0
    try:
        return float(total)
    except OverflowError:
        return math.inf if total > 0 else -math.inf


def exact_square(x):
    x = float(x)
    if math.isnan(x):
        return math.nan
    if math.isinf(x):
        return math.inf
    return float(Fraction(x) * Fraction(x))  # (a float32 squared is exact in binary64: nothing rounds here)


SPECIALS = np.array([0.0, -0.0, 1.0e-45, -1.0e-45, 1.1754942e-38, 2.0 ** 60, 2.0 ** -60, -(2.0 ** 60), 1.0, 1.0 + 2.0 ** -23, 3.4028235e38,
                     np.inf, -np.inf, np.nan, 0.1, -0.3], np.float32)


def crafted_frames(frame_count, pixel_count, seed):
    """float32 frames (pixels, 4): every special meets every other one across frames, the rest covers the exponent range"""
    rng = np.random.default_rng(seed)
    frames = []
    for _ in range(frame_count):
        x = (rng.standard_normal((pixel_count, 4)) * np.exp2(rng.integers(-70, 70, (pixel_count, 4)))).astype(np.float32)
        where = rng.random((pixel_count, 4)) < 0.5
        x[where] = rng.choice(SPECIALS, int(where.sum()))
        frames.append(x)
    return frames


def test_accumulation_equals_exact_rational_arithmetic_rounded_once_per_addition():
    frames = crafted_frames(7, 48, 1)
    # two pixels that hold -0 in every frame, and terms 2^+-60 apart
    for x in frames:
        x[0, :] = -0.0
        x[1, :3] = [2.0 ** 60, 2.0 ** -60, -(2.0 ** 60)]
    frames[3][1, :3] = [2.0 ** -60, 2.0 ** 60, 2.0 ** -60]
    sums, squares = fs.reference_accumulate(frames)
    assert sums.shape == squares.shape == (48, 3) and sums.dtype == np.float64
    expected_sums, expected_squares = np.zeros((48, 3)), np.zeros((48, 3))
    for p in range(48):
        for c in range(3):
            s, q = 0.0, 0.0
            for x in frames:
                s = exact_add(s, x[p, c])
                q = exact_add(q, exact_square(x[p, c]))
            expected_sums[p, c], expected_squares[p, c] = s, q
    nan = np.isnan(expected_sums)
    # (0 + -0 = +0: a sum that starts from +0 never becomes -0)
    assert nan.any() and np.isinf(expected_sums).any() and (bits(sums[0]) == 0).all()
    assert np.array_equal(np.isnan(sums), nan) and np.array_equal(bits(sums)[~nan], bits(expected_sums)[~nan])
    nan = np.isnan(expected_squares)
    assert np.array_equal(np.isnan(squares), nan) and np.array_equal(bits(squares)[~nan], bits(expected_squares)[~nan])
    # handing the frames over in two parts continues the same sums
    first = fs.reference_accumulate(frames[:3])
    again = fs.reference_accumulate(frames[3:], *first)
    assert np.array_equal(bits(again[0]), bits(sums)) and np.array_equal(bits(again[1]), bits(squares))


def exact_divide(a, b):
    return float(Fraction(a) / Fraction(b))


def test_mean_and_variance_equal_exact_rational_arithmetic_rounded_once_per_operation():
    rng = np.random.default_rng(2)
    frames = [(rng.random((40, 4)) * np.exp2(rng.integers(-20, 20, (40, 1)))).astype(np.float32) for _ in range(5)]
    sums, squares = fs.reference_accumulate(frames)
    mean, variance = fs.reference_mean_variance(sums, squares, 5)
    assert mean.dtype == variance.dtype == np.float32 and mean.shape == variance.shape == (40, 4)
    assert (mean[:, 3] == 1).all() and (variance[:, 3] == 1).all()
    for p in range(40):
        for c in range(3):
            s, q = float(sums[p, c]), float(squares[p, c])
            assert mean[p, c] == np.float32(exact_divide(s, 5))
            square = float(Fraction(s) * Fraction(s))
            difference = float(Fraction(q) - Fraction(exact_divide(square, 5)))
            v = exact_divide(difference, 4)
            assert variance[p, c] == np.float32(max(v, 0.0))


def test_variance_edge_cases():
    # cancellation: equal samples whose S * S / n rounds above Q
    x = np.float32(0.1)
    found = False
    for n in range(2, 40):
        sums, squares = fs.reference_accumulate([np.full((1, 4), x, np.float32)] * n)
        raw = (squares - sums * sums / n) / (n - 1)
        mean, variance = fs.reference_mean_variance(sums, squares, n)
        assert (variance[:, :3] >= 0).all()
        if (raw < 0).any():
            found = True
            assert (variance[:, :3][raw < 0] == 0).all() and not np.signbit(variance[:, :3][raw < 0]).any()
    assert found, "no case with a negative raw variance"
    # NaN and -0 pass the clamp
    sums, squares = np.array([[np.nan, 0.0, 2.0]]), np.array([[1.0, -0.0, 2.0]])
    mean, variance = fs.reference_mean_variance(sums, squares, 2)
    assert np.isnan(variance[0, 0]) and np.isnan(mean[0, 0])
    assert variance[0, 1] == 0 and np.signbit(variance[0, 1])  # (-0 - 0 / 2) / 1 = -0
    assert variance[0, 2] == 0 and not np.signbit(variance[0, 2])  # (2 - 4 / 2) / 1 = +0
    inf_sums, inf_squares = fs.reference_accumulate([np.full((1, 4), np.inf, np.float32), np.ones((1, 4), np.float32)])
    mean, variance = fs.reference_mean_variance(inf_sums, inf_squares, 2)
    assert np.isinf(mean[0, 0]) and np.isnan(variance[0, 0])  # inf - inf
    # fewer than two frames have no variance
    mean, variance = fs.reference_mean_variance(np.ones((1, 3)), np.ones((1, 3)), 1)
    assert variance is None and (mean == 1).all()
    with pytest.raises(ValueError):
        fs.reference_mean_variance(np.ones((1, 3)), np.ones((1, 3)), 0)


def slot_rule(terms):
    """The order of additions of include/vkr_frame_statistics.h as a plain loop"""
    partials = []
    for first in range(0, max(len(terms), 1), 256):
        slot = [float(v) for v in terms[first:first + 256]]
        slot += [0.0] * (256 - len(slot))
        s = 128
        while s:
            for j in range(s):
                slot[j] = exact_add(slot[j], slot[j + s])
            s //= 2
        partials.append(slot[0])
    total = 0.0
    for partial in partials:
        total = exact_add(total, partial)
    return total


@pytest.mark.parametrize("count", [1, 255, 256, 257, 1000])
def test_tree_sum_follows_the_slot_rule(count):
    rng = np.random.default_rng(count)
    terms = rng.standard_normal(count) * np.exp2(rng.integers(-40, 40, count))
    terms[rng.random(count) < 0.1] = 0.0
    terms[rng.random(count) < 0.05] = -0.0
    assert bits(fs.reference_tree_sum(terms)) == bits(slot_rule(terms))
    # several channels at once are the channels one by one
    channels = np.stack([terms, terms[::-1], np.abs(terms)], axis=1)
    together = fs.reference_tree_sum(channels)
    assert together.shape == (3,)
    assert np.array_equal(bits(together), bits([slot_rule(channels[:, c]) for c in range(3)]))
    # all -0 terms: the padding and the initial value are +0
    assert bits(fs.reference_tree_sum(np.full(count, -0.0))) == bits(0.0)
    # non-finite terms propagate
    special = terms.copy()
    special[count // 2] = np.inf
    assert fs.reference_tree_sum(special) == np.inf
    special[0] = -np.inf
    assert np.isnan(fs.reference_tree_sum(special)) or count == 1


@pytest.mark.parametrize("count", [1, 255, 256, 257, 1000])
def test_tree_sum_of_non_negative_terms_is_close_to_the_exact_sum(count):
    """A term passes through at most 8 rounded additions inside its block and one per block after it - at most
    11 for these counts.  With u = 2^-53 and non-negative terms the computed sum is therefore within
    gamma_11 = 11 u / (1 - 11 u) relative of the exact one, and math.fsum within u / 2 of it: together far inside
    (count - 1) u for count >= 255.  One term is added to zeros only: exact, the bound 0."""
    rng = np.random.default_rng(100 + count)
    terms = rng.random(count) * np.exp2(rng.integers(-30, 30, count))
    exact = math.fsum(terms)
    assert abs(float(fs.reference_tree_sum(terms)) - exact) <= (count - 1) * 2.0 ** -53 * exact


def test_error_terms():
    a, b = crafted_frames(2, 64, 3)
    d = fs.squared_difference_terms(a, b)
    assert d.shape == (64, 3) and d.dtype == np.float64
    for p in range(64):
        for c in range(3):
            x, y = float(a[p, c]), float(b[p, c])
            difference = exact_add(x, -y)
            # (|difference| < 2^129: its square is far from overflow)
            expected = float(Fraction(difference) * Fraction(difference)) if math.isfinite(difference) else abs(difference)
            assert (math.isnan(expected) and math.isnan(d[p, c])) or bits(d[p, c]) == bits(expected)
    assert np.array_equal(bits(fs.frame_terms(a)), bits(a[:, :3].astype(np.float64)))
    assert bits(fs.reference_tree_sum(fs.squared_difference_terms(np.ones((300, 4), np.float32), np.ones((300, 4), np.float32)))).tolist() == [0, 0, 0]


def test_struct_mirror_and_symbols():
    lib = capi.load()
    sizes = (C.c_uint64 * 32)()
    count = lib.get_abi_struct_sizes(sizes, 32)
    assert count == len(capi.ABI_STRUCTS) and capi.ABI_STRUCTS[-1] is capi.FrameStatistics
    assert sizes[count - 1] == C.sizeof(capi.FrameStatistics)
    assert len(capi.FrameStatistics().accumulated) == 2 * capi.MAX_ACCUMULATED_FRAMES
    for name in ("create_frame_statistics", "destroy_frame_statistics", "reset_frame_statistics", "accumulate_frames",
                 "resolve_frame_statistics", "read_back_frame_statistics", "sum_squared_differences", "sum_frame"):
        assert hasattr(lib, name) and name in capi.SIGNATURES


def test_requests_that_need_no_device_are_refused_with_a_message(capfd):
    """The argument checks come before any HIP call"""
    lib = capi.load()
    app = capi.Application()
    stats = capi.FrameStatistics()
    # no pixel count and no swapchain extent
    assert lib.create_frame_statistics(C.byref(stats), C.byref(app), 0) == 1
    assert not stats.sums
    # an object that was never created
    assert lib.accumulate_frames(C.byref(stats), C.byref(app), None, 1) == 1
    assert lib.resolve_frame_statistics(C.byref(stats), C.byref(app), None, None) == 1
    out = (C.c_double * 3)()
    assert lib.sum_frame(C.byref(app), None, 16, out) == 1
    assert lib.sum_squared_differences(C.byref(app), None, None, 16, out) == 1
    lib.destroy_frame_statistics(C.byref(stats), C.byref(app))
