"""The frame filter (include/vkr_frame_filter.h) without a GPU: the numpy restatement (vulkan_renderer_amd/frame_filter.py)
against a plain per-pixel loop in binary64, its exp2_poly against the oracle's vkr_exp2f, properties of the rule, the
conditions of the cases of tests/frame_filter_cases.py, the ctypes mirror and the refusals that need no device."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import frame_filter_cases as cases
from helpers import flush_c_output
from vulkan_renderer_amd import capi, frame_filter

f32 = np.float32
U = 2.0 ** -24  # unit roundoff of binary32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = (0.375, 0.25, 0.0625)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_cases_meet_their_conditions(name):
    cases.assert_conditions(name)


# ---- the restatement against a plain loop ----------------------------------------------------------------------------

def lum64(c):
    return 0.2126 * c[0] + 0.7152 * c[1] + 0.0722 * c[2]


def loop_iteration(c, v, position, normal, step, settings):
    """One iteration of the rule, pixel by pixel in binary64, for non-negative colours and variances -> (c', v', bound on
    |c' - c'_32|, bound on |v' - v'_32|) where x_32 is what binary32 with every operation rounded on its own gives from the
    same inputs, to first order in U:
      dot(n_p, n_q) = d: 3 U S with S the sum of the absolute products; k squarings: 2^k (3 U S / d + U) relative
      e_z: the differences U each, the dot 3 U of the absolute products, then d_z and the quotient: 4 U A / d_z + 2 U e_z
      l: 3 U (positive terms); |l_q - l_p|: 3 U (l_q + l_p) + U of itself
      d_l: eight additions of positive terms, a quotient, a root (halves, rounds), a luminance, a product, a sum: 12 U
      e_l: 3 U (l_q + l_p) / d_l + 14 U e_l
      t: 1.4427 (de_z + de_l) + 2 U |t|;  w_e: 4 U (the polynomial: relative error < 2e-7) + ln 2 dt
      w: rho = the sum of the above + 2 U, relative
      sums of n <= 25 positive terms: each term rho + U, the additions 24 U;  quotients U."""
    height, width = c.shape[:2]
    k = int(settings["normal_squarings"])
    out_c, out_v = np.zeros((height, width, 3)), np.zeros((height, width, 3))
    bound_c, bound_v = np.zeros((height, width, 3)), np.zeros((height, width, 3))
    for y in range(height):
        for x in range(width):
            if not position[y, x, 3] > 0:
                continue
            n_p, P_p, c_p = normal[y, x, :3], position[y, x, :3], c[y, x]
            l_p = lum64(c_p)
            d_l = None
            if v is not None:
                sum_gv, sum_g = np.zeros(3), 0.0
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        qx, qy = x + dx, y + dy
                        if 0 <= qx < width and 0 <= qy < height and position[qy, qx, 3] > 0:
                            g = (0.5 if dx == 0 else 0.25) * (0.5 if dy == 0 else 0.25)
                            sum_gv, sum_g = sum_gv + g * v[qy, qx], sum_g + g
                d_l = float(settings["sigma_luminance"]) * lum64(np.sqrt(sum_gv / sum_g)) + float(f32(1.0e-8))
            d_z = float(f32(settings["sigma_depth"])) * position[y, x, 3]
            sum_c, sum_v, sum_w = np.zeros(3), np.zeros(3), 0.0
            error_c, error_v, error_w = np.zeros(3), np.zeros(3), 0.0
            for dy in (-2, -1, 0, 1, 2):
                for dx in (-2, -1, 0, 1, 2):
                    qx, qy = x + dx * step, y + dy * step
                    if not (0 <= qx < width and 0 <= qy < height and position[qy, qx, 3] > 0):
                        continue
                    w, rho = KERNEL[abs(dx)] * KERNEL[abs(dy)], 0.0
                    if dx or dy:
                        d = float(np.dot(n_p, normal[qy, qx, :3]))
                        if not d > 0:
                            continue
                        S = float(np.abs(n_p * normal[qy, qx, :3]).sum())
                        rho = 2.0 ** k * (3.0 * U * S / d + U)
                        dP = position[qy, qx, :3] - P_p
                        e_z = abs(float(np.dot(n_p, dP))) / d_z
                        de = 4.0 * U * float(np.abs(n_p * dP).sum()) / d_z + 2.0 * U * e_z
                        e = e_z
                        if v is not None:
                            l_q = lum64(c[qy, qx])
                            e_l = abs(l_q - l_p) / d_l
                            de += 3.0 * U * (l_q + l_p) / d_l + 14.0 * U * e_l
                            e += e_l
                        t = -e * float(f32(1.44269502))
                        if not t >= -126.0:
                            continue
                        rho += 4.0 * U + math.log(2.0) * (float(f32(1.44269502)) * de + 2.0 * U * abs(t)) + 2.0 * U
                        w = w * d ** (2 ** k) * 2.0 ** t
                    sum_c, sum_w = sum_c + w * c[qy, qx], sum_w + w
                    error_c, error_w = error_c + w * c[qy, qx] * (rho + U), error_w + w * rho
                    if v is not None:
                        sum_v, error_v = sum_v + w * w * v[qy, qx], error_v + w * w * v[qy, qx] * (2.0 * rho + 2.0 * U)
            error_c, error_v, error_w = error_c + 24.0 * U * sum_c, error_v + 24.0 * U * sum_v, error_w + 24.0 * U * sum_w
            out_c[y, x] = sum_c / sum_w
            bound_c[y, x] = (error_c + out_c[y, x] * error_w) / sum_w + U * out_c[y, x]
            if v is not None:
                out_v[y, x] = sum_v / (sum_w * sum_w)
                bound_v[y, x] = (error_v + out_v[y, x] * (2.0 * error_w * sum_w + U * sum_w * sum_w)) / (sum_w * sum_w) + U * out_v[y, x]
    return out_c, (out_v if v is not None else None), bound_c, bound_v


@pytest.mark.parametrize("name", ["7x3", "16x16"])
def test_restatement_equals_a_plain_loop_within_its_roundings(name):
    """Every iteration on its own: the binary32 inputs that the restatement gives iteration i go through the loop in binary64,
    and the restatement's output of that iteration lies within the bound that the loop derives from the operation count (1 %
    more for the terms beyond first order; a tap whose weight one of the two flushes to zero is below 2^-126 of the kernel:
    1e-30 absolute).  Prepare and finish are single operations: U per operation."""
    images = cases.inputs(name)
    settings = frame_filter.check_settings(cases.settings(name))
    position, normal = images["position"], images["normal"]
    covered = position[..., 3] > 0
    c, v = images["colour"][..., :3], images["variance"][..., :3] * f32(settings["variance_scale"])
    assert (c[covered] >= 0).all() and (v[covered] >= 0).all()
    if images["modulation"] is not None:
        m = frame_filter.gmax(images["modulation"][..., :3], f32(1.0 / 256.0))
        m64 = np.maximum(images["modulation"][..., :3].astype(np.float64), 1.0 / 256.0)
        c0, v0 = c / m, v / (m * m)
        assert (np.abs(c0 - c.astype(np.float64) / m64) <= U * np.abs(c0)).all()
        assert (np.abs(v0 - v.astype(np.float64) / (m64 * m64)) <= 2.0 * U * np.abs(v0)).all()
        c, v = c0, v0
    worst = 0.0
    for i in range(settings["iteration_count"]):
        got_c, got_v = frame_filter.iteration(c, v, position, normal, covered, 1 << i, settings)
        want_c, want_v, bound_c, bound_v = loop_iteration(c.astype(np.float64), v.astype(np.float64), position.astype(np.float64),
                                                          normal.astype(np.float64), 1 << i, settings)
        for got, want, bound in ((got_c, want_c, bound_c), (got_v, want_v, bound_v)):
            difference = np.abs(got.astype(np.float64) - want)[covered]
            allowed = 1.01 * bound[covered] + 1.0e-30
            worst = max(worst, float((difference / allowed).max()))
            assert (difference <= allowed).all(), (i, float((difference / allowed).max()))
        c, v = got_c, got_v
    print(name, "largest difference / bound: %.3f" % worst)
    # (a bound that is orders of magnitude above the differences would show nothing)
    assert worst > 1.0e-3


# ---- exp2_poly -------------------------------------------------------------------------------------------------------

EXP2_SHIM = """
#include "oracle/oracle_math.h"
int g_oracle_system_libm = 0;
int g_oracle_math_mode = 0;
void shim_exp2(const float* t, float* out, int count) {
	for (int i = 0; i != count; ++i) out[i] = vkr_exp2f(t[i]);
}
"""


def test_exp2_poly_equals_the_oracle_bit_for_bit(tmp_path):
    """vkr_exp2f of oracle/oracle_math.h is a static function that no export of the oracle library reaches, so the header
    is compiled here as it is, with the flags of oracle/Makefile, behind a three-line export"""
    source, library = tmp_path / "exp2_shim.c", tmp_path / "libexp2_shim.so"
    source.write_text(EXP2_SHIM)
    subprocess.check_call([os.environ.get("CC", "gcc"), "-O2", "-std=gnu99", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-fPIC", "-shared",
                           "-Wno-unused-function", "-I", ROOT, str(source), "-o", str(library), "-lm"])
    shim = C.CDLL(str(library))
    rng = np.random.default_rng(11)
    integers = np.arange(-126, 1, dtype=f32)
    t = np.concatenate([integers, np.nextafter(integers[:-1], f32(np.inf)), np.nextafter(integers[1:], f32(-np.inf)), integers[1:] - f32(0.5),
                        rng.uniform(-126.0, 0.0, 4000).astype(f32), -np.exp2(rng.uniform(-30.0, 0.0, 500)).astype(f32), np.array([-0.0], f32)])
    assert ((t >= -126) & (t <= 0)).all() and len(t) > 4000
    want = np.zeros_like(t)
    pointer = C.POINTER(C.c_float)
    shim.shim_exp2(t.ctypes.data_as(pointer), want.ctypes.data_as(pointer), len(t))
    got = frame_filter.exp2_poly(t)
    assert got.dtype == f32 and got.tobytes() == want.tobytes()
    # what it is: 2^t (the polynomial's relative error is below 2e-7; one more rounding for the scale)
    assert (np.abs(got.astype(np.float64) / np.exp2(t.astype(np.float64)) - 1.0) < 3.0e-7).all()
    assert got[0] == f32(2.0 ** -126) and got[126] == 1.0


def test_fma32_rounds_once():
    rng = np.random.default_rng(12)
    a, b = rng.standard_normal(20000).astype(f32), rng.standard_normal(20000).astype(f32)
    c = (-(a.astype(np.float64) * b) * (1.0 + rng.standard_normal(20000) * 1.0e-7)).astype(f32)
    got = frame_filter.fma32(a, b, c)
    # the exact value a * b + c as a sum of two doubles, rounded once to binary32 by way of exact rational arithmetic
    from fractions import Fraction
    for i in range(0, 20000, 97):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        low, high = (f32(got[i]), np.nextafter(got[i], f32(np.inf))) if Fraction(float(got[i])) <= exact else (np.nextafter(got[i], f32(-np.inf)), f32(got[i]))
        nearest = low if exact - Fraction(float(low)) < Fraction(float(high)) - exact else high
        if exact - Fraction(float(low)) == Fraction(float(high)) - exact:
            nearest = low if (int(np.array(low, f32).view(np.uint32)) & 1) == 0 else high
        assert got[i] == nearest, i


# ---- properties of the rule ------------------------------------------------------------------------------------------

def flat_frame(width, height):
    """A plane z = 4 that faces the origin, all covered; coordinates with short significands: every dot product is exact"""
    ys, xs = np.mgrid[0:height, 0:width]
    position = np.stack([xs * 0.125, ys * 0.125, np.full((height, width), 4.0), np.full((height, width), 4.5)], axis=-1).astype(f32)
    normal = np.zeros((height, width, 4), f32)
    normal[..., 2] = 1.0
    return position, normal


def test_a_constant_image_comes_back_unchanged():
    """On a flat plane under a constant colour every e_z and e_l is 0, exp2_poly(-0) is 1 and w = h, a multiple of 1 / 256.
    With a colour of at most eight significant bits every product w * c and every partial sum is exact, so c' = c in every
    bit, at the borders too (fewer taps, the same argument).  The variance does not enter."""
    position, normal = flat_frame(37, 21)
    colour = np.zeros((21, 37, 4), f32)
    colour[...] = (0.75, 1.5, 0.3125, 7.0)
    variance = np.zeros_like(colour)
    variance[...] = (0.01, 0.02, 0.03, 1.0)
    for with_variance in (True, False):
        out, out_variance = frame_filter.filter_frame(colour, variance if with_variance else None, position, normal, None, dict(cases.SETTINGS, iteration_count=5))
        assert out.tobytes() == colour.tobytes()
        assert (out_variance is not None) == with_variance


def test_flat_region_variance_after_one_iteration():
    """All 25 weights are h there: v' = v * sum(h^2) / (sum h)^2 = v * (70 / 256)^2 / 1, exactly for a short v"""
    position, normal = flat_frame(20, 12)
    colour = np.zeros((12, 20, 4), f32)
    colour[..., :3] = 0.5
    variance = np.zeros_like(colour)
    variance[...] = (0.25, 0.5, 0.0078125, 1.0)
    out, out_variance = frame_filter.filter_frame(colour, variance, position, normal, None, dict(cases.SETTINGS, iteration_count=1))
    sum_h2 = sum((a * b) ** 2 for a in (0.0625, 0.25, 0.375, 0.25, 0.0625) for b in (0.0625, 0.25, 0.375, 0.25, 0.0625))
    sum_h = sum(a * b for a in (0.0625, 0.25, 0.375, 0.25, 0.0625) for b in (0.0625, 0.25, 0.375, 0.25, 0.0625))
    assert sum_h == 1.0 and sum_h2 == (70.0 / 256.0) ** 2
    interior = out_variance[2:-2, 2:-2, :3]
    assert np.array_equal(interior, np.broadcast_to((variance[0, 0, :3].astype(np.float64) * sum_h2).astype(f32), interior.shape))
    # fewer taps at the border: less averaging
    assert (out_variance[0, 0, :3] > interior[0, 0]).all() and (out_variance[..., 3] == 1).all()


def two_planes(width=48, height=32, sigma=0.05, seed=21):
    """The valley without its extras: 0.2 on the left of the crease, 0.8 on the right, noise of `sigma`, its variance"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:height, 0:width]
    crease = width // 2
    X = ((xs - crease) * 0.1).astype(f32)
    Z = (f32(5.0) + f32(0.75) * np.abs(X)).astype(f32)
    Y = (ys * 0.1).astype(f32)
    position = np.stack([X, Y, Z, np.sqrt((X * X + Y * Y) + Z * Z)], axis=-1).astype(f32)
    left = xs < crease
    normal = np.zeros((height, width, 4), f32)
    normal[..., :3] = np.where(left[..., None], cases.N1, cases.N2)
    clean = np.zeros((height, width, 4), f32)
    clean[..., :3] = np.where(left, 0.2, 0.8)[..., None]
    colour = clean.copy()
    colour[..., :3] += (sigma * rng.standard_normal((height, width, 1))).astype(f32)
    variance = np.full((height, width, 4), sigma * sigma, f32)
    return colour, variance, position, normal, clean, left


def test_the_error_falls_inside_each_plane_and_nothing_crosses_the_crease():
    """Across the crease the normal weight is 0.28^256 = 0, so a pixel's value is a convex combination of the noisy values of
    its own side: it cannot leave their range, whatever the noise, but for the roundings - each of at most 25 products and 25
    additions of positive terms and the quotient, per iteration: 51 U relative, five times.  And the mean squared error
    against the noise-free image falls on either side; averaging 25 equal-variance pixels would divide it by 1 / 0.0748 = 13,
    the luminance weight keeps it lower: the test asks for a factor of 4."""
    colour, variance, position, normal, clean, left = two_planes()
    out, out_variance = frame_filter.filter_frame(colour, variance, position, normal, None, dict(cases.SETTINGS, iteration_count=5))
    slack = 1.0 + 5 * 51 * U
    for side in (left, ~left):
        noisy, filtered = colour[..., :3][side].astype(np.float64), out[..., :3][side].astype(np.float64)
        assert filtered.max() <= noisy.max() * slack and filtered.min() >= noisy.min() / slack
        before = ((noisy - clean[..., :3][side]) ** 2).mean()
        after = ((filtered - clean[..., :3][side]) ** 2).mean()
        print("mean squared error %.3e -> %.3e" % (before, after))
        assert after < before / 4.0
        assert (out_variance[..., :3][side] < variance[..., :3][side]).all()
    # the two sides stay apart by more than the noise ever reached
    assert out[..., 0][left].max() < 0.5 < out[..., 0][~left].min()


# ---- the binding -----------------------------------------------------------------------------------------------------

def test_ctypes_mirror():
    header = open(os.path.join(ROOT, "include", "vkr_frame_filter.h")).read()
    for struct, mirror in (("frame_filter_settings_s", capi.FrameFilterSettings), ("frame_filter_images_s", capi.FrameFilterImages), ("frame_filter_s", capi.FrameFilter)):
        body = re.search(r"typedef struct %s \{(.*?)\n\} \w+;" % struct, header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        members = []
        for declaration in body.split(";"):
            declaration = declaration.strip()
            if not declaration:
                continue
            kind = declaration.rsplit(None, 1)[0] if "," not in declaration else declaration.split(None, 1)[0]
            for name in declaration[len(kind):].split(","):
                name = name.strip().lstrip("*")
                count = re.search(r"\[(\d+)\]", name)
                members.append((name.split("[")[0], kind.strip(), int(count.group(1)) if count else None))
        assert [m[0] for m in members] == [f[0] for f in mirror._fields_], struct
        for (name, kind, count), field in zip(members, mirror._fields_):
            base = {"uint32_t": C.c_uint32, "float": C.c_float}.get(kind, C.c_void_p)
            assert field[1] == (base * count if count else base), (struct, name)
    assert C.sizeof(capi.FrameFilterSettings) == 20 and C.sizeof(capi.FrameFilterImages) == 56 and C.sizeof(capi.FrameFilter) == 48
    for constant, value in (("MAX_ITERATIONS", capi.FRAME_FILTER_MAX_ITERATIONS), ("MAX_NORMAL_SQUARINGS", capi.FRAME_FILTER_MAX_NORMAL_SQUARINGS),
                            ("MAX_EXTENT", capi.FRAME_FILTER_MAX_EXTENT)):
        assert int(re.search(r"#define VKR_FRAME_FILTER_%s (\d+)" % constant, header).group(1)) == value
    assert (frame_filter.MAX_ITERATIONS, frame_filter.MAX_NORMAL_SQUARINGS) == (capi.FRAME_FILTER_MAX_ITERATIONS, capi.FRAME_FILTER_MAX_NORMAL_SQUARINGS)
    lib = capi.load()
    for symbol in ("create_frame_filter", "filter_frame"):
        assert "VKR_API int %s(" % symbol in header
        assert hasattr(lib, symbol) and symbol in capi.SIGNATURES
    assert "VKR_API void destroy_frame_filter(" in header and hasattr(lib, "destroy_frame_filter") and "destroy_frame_filter" in capi.SIGNATURES


def test_refusals_that_need_no_device(capfd):
    """Settings, the variance output and the pointers are looked at before the filter and the device: each refusal returns 1
    and prints one line"""
    lib = capi.load()
    app, filter_ = capi.Application(), capi.FrameFilter()
    good = dict(iteration_count=3, normal_squarings=7, sigma_luminance=4.0, sigma_depth=0.02, variance_scale=0.25)
    pointers = dict(colour=0x1000, variance=0x2000, position=0x3000, normal=0x4000, modulation=0x5000, out_colour=0x6000, out_variance=0x7000)
    nan, inf = float("nan"), float("inf")

    def refused(settings, images):
        s = capi.FrameFilterSettings(*[dict(good, **settings)[name] for name, _ in capi.FrameFilterSettings._fields_])
        i = capi.FrameFilterImages(*[dict(pointers, **images)[name] for name, _ in capi.FrameFilterImages._fields_])
        flush_c_output()
        capfd.readouterr()
        assert lib.filter_frame(C.byref(filter_), C.byref(app), C.byref(s), C.byref(i)) == 1, (settings, images)
        flush_c_output()
        printed = capfd.readouterr().out
        assert printed.count("\n") == 1 and printed.endswith("\n") and len(printed) > 20, (settings, images, printed)
        return printed

    for settings in [dict(iteration_count=0), dict(iteration_count=6), dict(iteration_count=0xFFFFFFFF), dict(normal_squarings=9),
                     dict(sigma_luminance=0.0), dict(sigma_luminance=-1.0), dict(sigma_luminance=nan), dict(sigma_luminance=inf),
                     dict(sigma_depth=0.0), dict(sigma_depth=nan), dict(sigma_depth=inf), dict(variance_scale=-0.5), dict(variance_scale=nan),
                     dict(variance_scale=inf)]:
        assert "iterations" in refused(settings, {})
    assert "variance" in refused({}, dict(variance=None))
    for images in [dict(colour=None), dict(position=None), dict(normal=None), dict(out_colour=None), dict(colour=0x1004), dict(variance=0x2008),
                   dict(position=0x3001), dict(normal=0x400C), dict(modulation=0x5002), dict(out_colour=0x6004), dict(out_variance=0x7008)]:
        assert "16-byte aligned" in refused({}, images)
    # nothing wrong but the filter, which was never created
    assert "create_frame_filter" in refused({}, {})
    assert "create_frame_filter" in refused(dict(variance_scale=0.0, normal_squarings=0, iteration_count=1), dict(variance=None, out_variance=None, modulation=None))
    # an extent that is none
    for width, height in ((0, 0), (0, 5), (5, 0), (capi.FRAME_FILTER_MAX_EXTENT + 1, 4), (4, 0xFFFFFFFF)):
        flush_c_output()
        capfd.readouterr()
        assert lib.create_frame_filter(C.byref(filter_), C.byref(app), width, height) == 1
        flush_c_output()
        assert capfd.readouterr().out.count("\n") == 1
        assert not filter_.filtered and not filter_.colour_scratch[0]
    with pytest.raises(ValueError):
        frame_filter.check_settings(dict(iteration_count=6))
    with pytest.raises(ValueError):
        frame_filter.check_settings(dict(sigma_depth=nan))
