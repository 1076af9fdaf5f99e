"""The frame history (include/vkr_frame_history.h) without a GPU: the conditions of the sequences of
tests/frame_history_cases.py, the numpy restatement (vulkan_renderer_amd/frame_history.py) against a plain per-pixel loop in
binary64, properties of the rule, the ctypes mirror and the refusals that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import frame_history_cases as cases
from helpers import flush_c_output
from vulkan_renderer_amd import capi, frame_history

f32 = np.float32
U = 2.0 ** -24  # unit roundoff of binary32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(cases.SEQUENCES))
def test_sequences_meet_their_conditions(name):
    cases.assert_conditions(name)


def test_every_rejection_and_every_pixel_class_occurs_at_83x45():
    totals = cases.assert_every_reason_and_class_occurs()
    print(totals)
    # a pixel with too little weight that is usable, and one that is not usable
    assert totals["low_weight"] > 0 and totals["not_usable"] > 0 and totals["skipped_without_history"] > 0
    assert totals["skipped_sample"] > totals["skipped_without_history"]


def test_null_and_identity_reprojection_give_the_same_bytes():
    for a, b in zip(cases.expected("still_null"), cases.expected("still_identity")):
        assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
        assert all(a[0][key].tobytes() == b[0][key].tobytes() for key in frame_history.HISTORY_IMAGES)


# ---- the restatement against a plain loop ----------------------------------------------------------------------------

def dot64(a, b):
    return float(a[0] * b[0] + a[1] * b[1] + a[2] * b[2])


def loop_frame(state, frame, settings):
    """One call of the rule, pixel by pixel in binary64, for non-negative colours -> (c', s', n', out_colour, out_variance of
    the first launch, and a bound per value) at covered pixels with a finite sample; NaN elsewhere.  The bound is on the
    difference to what binary32 with every operation rounded on its own gives from the same inputs, to first order in U.
    The coordinates of the sequences are multiples of 1 / 16, so tx, 1 - tx, b and sum_b are exact (asserted), and the
    verdicts on the taps are far from their thresholds.  With e_c = U (with a modulation image: c = colour / m) or 0, and
    e_s = 2 e_c + U for s = c * c:
      sum_c: a product and at most three additions per term: 4 U sum_c (positive terms);  hc = sum_c / sum_b: 5 U, hs, n too
      n' = gmin(n + 1, L): 6 U;  a = 1 / n': 7 U
      d = c - hc: e_c c + 5 U hc + U |d|;  a * d: 8 U |a d| + a times that;  c' = hc + a d: 5 U hc + the former + U c'
          = 5 U hc + a (e_c c + 5 U hc + 9 U |d|) + U c';  s' likewise with e_s
      without history c' = c, s' = s: e_c c, e_s s;  n' = 1
      out_colour = c' m: the bound of c' times m + U c' m
      e = s' - c' c': that of s' + 2 c' that of c' + U c'^2 + U |e|;  1 / gmax(n', 1): 7 U;  v: that of e over n' + 8 U v
      v (m m): m m is one rounding, the product another: that of v times m^2 + 2 U v m^2"""
    height, width = frame["colour"].shape[:2]
    L, sigma_depth, threshold = float(f32(settings["max_length"])), float(f32(settings["sigma_depth"])), float(f32(settings["normal_threshold"]))
    names = ("c", "s", "n", "out_colour", "out_variance")
    value = {name: np.full((height, width, 1 if name == "n" else 3), np.nan) for name in names}
    bound = {name: np.full((height, width, 1 if name == "n" else 3), np.nan) for name in names}
    position, normal, colour = (frame[key].astype(np.float64) for key in ("position", "normal", "colour"))
    old = {key: state[key].astype(np.float64) for key in frame_history.HISTORY_IMAGES}
    for y in range(height):
        for x in range(width):
            if not position[y, x, 3] > 0:
                continue
            m, e_c = np.ones(3), 0.0
            if frame["modulation"] is not None:
                m, e_c = np.maximum(frame["modulation"][y, x, :3].astype(np.float64), 1.0 / 256.0), U
            c = colour[y, x, :3] / m
            if not np.isfinite(c).all():
                continue
            assert (c >= 0).all()
            s, e_s = c * c, 2.0 * e_c + U
            r = (float(x), float(y), 1.0, 1.0) if frame["reprojection"] is None else [float(v) for v in frame["reprojection"][y, x]]
            usable = state["frame_count"] > 0 and r[3] == 1.0 and -1.0 <= r[0] < width and -1.0 <= r[1] < height
            sum_b, sum_c, sum_s, sum_n = 0.0, np.zeros(3), np.zeros(3), 0.0
            if usable:
                fx, fy = int(np.floor(r[0])), int(np.floor(r[1]))
                tx, ty = r[0] - fx, r[1] - fy
                for k in range(4):
                    qx, qy = fx + (k & 1), fy + (k >> 1)
                    b = (tx if k & 1 else 1.0 - tx) * (ty if k >> 1 else 1.0 - ty)
                    assert float(f32(b)) == b and b * 256.0 == int(b * 256.0)
                    if not (0 <= qx < width and 0 <= qy < height and b > 0 and old["position"][qy, qx, 3] > 0):
                        continue
                    if not abs(dot64(normal[y, x], old["position"][qy, qx, :3] - position[y, x, :3])) <= sigma_depth * position[y, x, 3]:
                        continue
                    if not dot64(normal[y, x], old["normal"][qy, qx]) >= threshold:
                        continue
                    sum_b, sum_c, sum_s, sum_n = sum_b + b, sum_c + b * old["colour"][qy, qx, :3], sum_s + b * old["moments"][qy, qx, :3], sum_n + b * old["colour"][qy, qx, 3]
            if usable and sum_b >= 1.0 / 64.0:
                hc, hs, n = sum_c / sum_b, sum_s / sum_b, sum_n / sum_b
                new_n = min(n + 1.0, L)
                a = 1.0 / new_n
                new_c, new_s = hc + a * (c - hc), hs + a * (s - hs)
                bound_c = 5.0 * U * hc + a * (e_c * c + 5.0 * U * hc + 9.0 * U * np.abs(c - hc)) + U * new_c
                bound_s = 5.0 * U * hs + a * (e_s * s + 5.0 * U * hs + 9.0 * U * np.abs(s - hs)) + U * new_s
                bound_n = 6.0 * U * new_n
            else:
                new_c, new_s, new_n = c, s, 1.0
                bound_c, bound_s, bound_n = e_c * c, e_s * s, 0.0
            e = new_s - new_c * new_c
            bound_e = bound_s + 2.0 * new_c * bound_c + U * new_c * new_c + U * np.abs(e)
            scale = 1.0 / max(new_n, 1.0)
            v = np.maximum(0.0, e) * scale
            bound_v = bound_e * scale + 8.0 * U * v
            value["c"][y, x], value["s"][y, x], value["n"][y, x] = new_c, new_s, new_n
            bound["c"][y, x], bound["s"][y, x], bound["n"][y, x] = bound_c, bound_s, bound_n
            value["out_colour"][y, x], bound["out_colour"][y, x] = new_c * m, bound_c * m + U * new_c * m
            value["out_variance"][y, x], bound["out_variance"][y, x] = v * m * m, bound_v * m * m + 2.0 * U * v * m * m
    return value, bound


def loop_spatial(new_state, frame, settings):
    """The second launch in binary64 from the binary32 h' of the restatement -> (out_variance, bound, which pixels), NaN where
    the estimate is not taken.  M1 and M2: at most 48 additions of positive terms and a quotient: 49 U each;  e = M2 - M1 M1:
    49 U M2 + 99 U M1^2 + U |e|;  1 / n': U;  v: that of e over n' + 2 U v;  v (m m): 2 U v m^2 more"""
    height, width = frame["colour"].shape[:2]
    sigma_depth, threshold, spatial_length = float(f32(settings["sigma_depth"])), float(f32(settings["normal_threshold"])), float(int(settings["spatial_length"]))
    position, normal = frame["position"].astype(np.float64), frame["normal"].astype(np.float64)
    new_colour, new_moments = new_state["colour"].astype(np.float64), new_state["moments"].astype(np.float64)
    value, bound = np.full((height, width, 3), np.nan), np.full((height, width, 3), np.nan)
    for y in range(height):
        for x in range(width):
            length = new_colour[y, x, 3]
            if not (position[y, x, 3] > 0 and 0 < length < spatial_length):
                continue
            M1, M2, count = np.zeros(3), np.zeros(3), 0
            for dy in range(-3, 4):
                for dx in range(-3, 4):
                    qx, qy = x + dx, y + dy
                    if dx or dy:
                        if not (0 <= qx < width and 0 <= qy < height and position[qy, qx, 3] > 0 and new_colour[qy, qx, 3] > 0):
                            continue
                        if not abs(dot64(normal[y, x], position[qy, qx, :3] - position[y, x, :3])) <= sigma_depth * position[y, x, 3]:
                            continue
                        if not dot64(normal[y, x], normal[qy, qx]) >= threshold:
                            continue
                    M1, M2, count = M1 + new_colour[qy, qx, :3], M2 + new_moments[qy, qx, :3], count + 1
            M1, M2 = M1 / count, M2 / count
            e = M2 - M1 * M1
            bound_e = 49.0 * U * M2 + 99.0 * U * M1 * M1 + U * np.abs(e)
            v = np.maximum(0.0, e) / length
            m = np.ones(3) if frame["modulation"] is None else np.maximum(frame["modulation"][y, x, :3].astype(np.float64), 1.0 / 256.0)
            value[y, x], bound[y, x] = v * m * m, (bound_e / length + 2.0 * U * v) * m * m + 2.0 * U * v * m * m
    return value, bound


@pytest.mark.parametrize("name", ["7x3", "33x35", "saturating", "1x1_modulated"])
def test_restatement_equals_a_plain_loop_within_its_roundings(name):
    """Every frame on its own: the binary32 history that the restatement gives frame i goes through the loop in binary64 with
    frame i, and what the restatement makes of the same lies within the bound that the loop derives from the operation count
    (1 % more for the terms beyond first order, 1e-30 for a denormal).  The spatial estimate likewise, from the binary32
    h'; where it is taken, out_variance is its value, elsewhere the first launch's."""
    width, height, _ = cases.SEQUENCES[name]
    settings = frame_history.check_settings(cases.settings(name))
    state = frame_history.new_state(width, height)
    worst, compared = {}, 0
    for index, frame in enumerate(cases.build(name)):
        new_state, out_colour, out_variance = frame_history.accumulate(state, frame["colour"], frame["position"], frame["normal"], frame["reprojection"],
                                                                       frame["modulation"], settings)
        value, bound = loop_frame(state, frame, settings)
        spatial_value, spatial_bound = loop_spatial(new_state, frame, settings)
        spatial = ~np.isnan(spatial_value[..., 0])
        got = {"c": new_state["colour"][..., :3], "s": new_state["moments"][..., :3], "n": new_state["colour"][..., 3:], "out_colour": out_colour[..., :3],
               "out_variance": out_variance[..., :3]}
        compare = ~np.isnan(value["c"][..., 0])
        assert compare.sum() > 0 and (compare == (frame["position"][..., 3] > 0)).all()
        for key in got:
            want, allowed, where = value[key], bound[key], compare
            if key == "out_variance":
                want, allowed = np.where(spatial[..., None], spatial_value, want), np.where(spatial[..., None], spatial_bound, allowed)
            difference = np.abs(got[key].astype(np.float64) - want)[where]
            allowed = 1.01 * allowed[where] + 1.0e-30
            share = float((difference / allowed).max())
            worst[key] = max(worst.get(key, 0.0), share)
            assert (difference <= allowed).all(), (name, index, key, share)
            compared += int(where.sum())
        if int(settings["spatial_length"]) and index < 2:
            assert spatial.any()
        state = new_state
    print(name, "values compared: %d, largest difference / bound:" % compared, {key: round(share, 3) for key, share in worst.items()})
    # (a bound that is orders of magnitude above the differences would show nothing)
    assert max(worst.values()) > 1.0e-2


# ---- properties of the rule ------------------------------------------------------------------------------------------

def test_still_camera_gives_the_running_mean_and_counts_the_frames():
    """Without a reprojection image every pixel has one tap of weight 1: hc = (1 * c) / 1 is exact, n' is exactly the frame
    number (max_length 32 > 6), a = 1 / n' is one rounding, and c'_f = c'_(f-1) + a (c_f - c'_(f-1)) is the running mean
    but for: U |d| in d, 2 U |a d| in the product, U c' in the sum.  The error of frame f - 1 enters with the factor 1 - a."""
    name = "still_null"
    frames, results = cases.build(name), cases.expected(name)
    covered = frames[0]["position"][..., 3] > 0
    total, error, share = np.zeros(frames[0]["colour"][..., :3].shape), np.zeros(frames[0]["colour"][..., :3].shape), 0.0
    for index, (frame, (state, _, _, _)) in enumerate(zip(frames, results)):
        c = frame["colour"][..., :3].astype(np.float64)
        a = 1.0 / (index + 1)
        previous_mean = total / max(index, 1)
        total += c
        mean = total / (index + 1)
        error = (1.0 - a) * error + 3.0 * U * a * np.abs(c - previous_mean) + U * mean if index else np.zeros_like(mean)
        assert (state["colour"][..., 3][covered] == index + 1).all()
        difference = np.abs(state["colour"][..., :3].astype(np.float64) - mean)[covered]
        allowed = 1.01 * error[covered] + 1.0e-30
        assert (difference <= allowed).all(), index
        if index:
            share = max(share, float((difference / allowed).max()))
    print("largest difference / bound: %.3f" % share)
    assert share > 1.0e-2


def nan_frame(frame):
    colour = frame["colour"].copy()
    colour[..., :3] = np.nan
    return colour


def test_whole_pixel_motion_fetches_the_shifted_pixel_bit_for_bit():
    """Under (x + 3, y - 2) tap 0 has weight 1 and the others 0: hc = (1 * h) / 1.  A frame whose samples are all NaN leaves the
    history as it is, so h' of p is h of the shifted pixel in every bit where that tap counts, and empty elsewhere"""
    name = "whole"
    frames, results = cases.build(name), cases.expected(name)
    state = results[3][0]
    frame = frames[4]
    diagnostics = {}
    new_state, out_colour, out_variance = frame_history.accumulate(state, nan_frame(frame), frame["position"], frame["normal"], frame["reprojection"], None,
                                                                   cases.settings(name), diagnostics)
    height, width = frame["colour"].shape[:2]
    has_history = new_state["colour"][..., 3] > 0
    assert diagnostics["skipped_sample"] == diagnostics["covered"] and 0 < has_history.sum() == diagnostics["covered"] - diagnostics["no_history"]
    ys, xs = np.nonzero(has_history)
    assert (xs + 3 < width).all() and (ys - 2 >= 0).all()
    for key in ("colour", "moments"):
        assert new_state[key][ys, xs].tobytes() == state[key][ys - 2, xs + 3].tobytes()
        assert not new_state[key][~has_history].any()
    assert out_colour[..., :3][has_history].tobytes() == new_state["colour"][..., :3][has_history].tobytes()
    # lengths of more than one frame came along
    assert new_state["colour"][..., 3].max() == 4


def test_a_frame_that_is_not_finite_leaves_the_history_as_it_is():
    """Still camera: h' = h in colour and moments, and so frame after frame; fraction: h' is the reprojected h, the
    numerators of c' before the sample is blended in - the same sums, which a finite sample with a = 0 would leave too"""
    name = "still_null"
    frames, results = cases.build(name), cases.expected(name)
    state = results[2][0]
    for frame in frames[3:5]:
        new_state, _, _ = frame_history.accumulate(state, nan_frame(frame), frame["position"], frame["normal"], None, None, cases.settings(name))
        assert new_state["colour"].tobytes() == state["colour"].tobytes() and new_state["moments"].tobytes() == state["moments"].tobytes()
        assert new_state["frame_count"] == state["frame_count"] + 1
        state = new_state
    name = "fraction"
    frames, results = cases.build(name), cases.expected(name)
    state, frame = results[2][0], frames[3]
    infinite = frame["colour"].copy()
    infinite[..., 1] = np.inf
    kept = frame_history.accumulate(state, infinite, frame["position"], frame["normal"], frame["reprojection"], frame["modulation"], cases.settings(name))[0]
    # the same call with a sample that is finite and a history so long that binary32 cannot tell a from 0: c' = hc + 0 * (c - hc)
    long_state = dict(state, colour=state["colour"].copy())
    long_state["colour"][..., 3] *= f32(2.0 ** 100)
    blended = frame_history.accumulate(long_state, frame["colour"], frame["position"], frame["normal"], frame["reprojection"], frame["modulation"],
                                       dict(cases.settings(name), max_length=3.0e38))[0]
    has_history = kept["colour"][..., 3] > 0
    assert has_history.any() and np.isfinite(kept["colour"]).all()
    difference = np.abs(kept["colour"][..., :3][has_history].astype(np.float64) - blended["colour"][..., :3][has_history])
    # (a = 2^-100 or so: a * d is far below half an ulp of hc unless hc is 0)
    assert (difference <= 1.0e-25).all()
    assert kept["moments"][has_history].tobytes() == blended["moments"][has_history].tobytes() or (np.abs(kept["moments"].astype(np.float64) - blended["moments"])[has_history] <= 1.0e-25).all()


def flat_frame(width, height):
    """A plane z = 4 that faces the origin, all covered; coordinates with short significands: every dot product is exact"""
    ys, xs = np.mgrid[0:height, 0:width]
    position = np.stack([xs * 0.125, ys * 0.125, np.full((height, width), 4.0), np.full((height, width), 4.5)], axis=-1).astype(f32)
    normal = np.zeros((height, width, 4), f32)
    normal[..., 2] = 1.0
    return position, normal


@pytest.mark.parametrize("shift", [None, (3, -2), (2.25, -1.5)])
def test_a_constant_sequence_is_unchanged_in_every_bit_with_variance_zero(shift):
    """A colour of short significands, the same in every pixel and frame: the weights are multiples of 1 / 16, so every product
    b * c and every partial sum is exact, hc = c, c - hc = 0 and c' = c; s' = c * c likewise, s' - c' * c' = 0.  The spatial
    estimate sums at most 49 equal terms, exactly, and gives 0 too."""
    width, height = 37, 21
    position, normal = flat_frame(width, height)
    colour = np.zeros((height, width, 4), f32)
    colour[...] = (0.75, 1.5, 0.3125, 7.0)
    reprojection = None if shift is None else cases.shift_image(width, height, *shift)
    state = frame_history.new_state(width, height)
    lengths = []
    for index in range(6):
        diagnostics = {}
        state, out_colour, out_variance = frame_history.accumulate(state, colour, position, normal, reprojection, None, cases.SETTINGS, diagnostics)
        assert out_colour.tobytes() == colour.tobytes()
        assert not out_variance[..., :3].any() and (out_variance[..., 3] == 1).all()
        assert state["colour"][..., :3].tobytes() == colour[..., :3].tobytes()
        assert (diagnostics["spatial"] > 0) == (index < 3 or shift is not None)
        lengths.append(float(state["colour"][..., 3].max()))
    assert lengths == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]


# ---- the binding -----------------------------------------------------------------------------------------------------

def test_ctypes_mirror():
    header = open(os.path.join(ROOT, "include", "vkr_frame_history.h")).read()
    for struct, mirror in (("frame_history_settings_s", capi.FrameHistorySettings), ("frame_history_images_s", capi.FrameHistoryImages),
                           ("frame_history_s", capi.FrameHistory)):
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
    assert C.sizeof(capi.FrameHistorySettings) == 16 and C.sizeof(capi.FrameHistoryImages) == 56 and C.sizeof(capi.FrameHistory) == 88
    assert int(re.search(r"#define VKR_FRAME_HISTORY_MAX_SPATIAL_LENGTH (\d+)", header).group(1)) == capi.FRAME_HISTORY_MAX_SPATIAL_LENGTH == frame_history.MAX_SPATIAL_LENGTH
    assert "#define VKR_FRAME_HISTORY_MAX_EXTENT VKR_FRAME_FILTER_MAX_EXTENT" in header and capi.FRAME_HISTORY_MAX_EXTENT == capi.FRAME_FILTER_MAX_EXTENT
    lib = capi.load()
    for symbol in ("create_frame_history", "accumulate_frame_history"):
        assert "VKR_API int %s(" % symbol in header
        assert hasattr(lib, symbol) and symbol in capi.SIGNATURES
    for symbol in ("destroy_frame_history", "reset_frame_history"):
        assert "VKR_API void %s(" % symbol in header and hasattr(lib, symbol) and symbol in capi.SIGNATURES


def test_refusals_that_need_no_device(capfd):
    """Settings, pointers, the history and the overlaps are looked at before the device: each refusal returns 1 and prints one
    line.  (The history of the overlap checks is made up of addresses that nothing is behind: no call gets as far as them.)"""
    lib = capi.load()
    app, empty = capi.Application(), capi.FrameHistory()
    good = dict(max_length=16.0, sigma_depth=0.02, normal_threshold=0.9, spatial_length=4)
    pointers = dict(colour=0x10000, position=0x20000, normal=0x30000, reprojection=0x40000, modulation=0x50000, out_colour=0x60000, out_variance=0x70000)
    nan, inf = float("nan"), float("inf")
    made_up = capi.FrameHistory()
    made_up.width, made_up.height, made_up.accumulated = 8, 8, 0xF0000
    for i, key in enumerate(frame_history.HISTORY_IMAGES):
        for j in range(2):
            getattr(made_up, key)[j] = 0x100000 + (2 * i + j) * 0x10000
    image_bytes = 8 * 8 * 16

    def refused(settings, images, history=empty):
        s = capi.FrameHistorySettings(*[dict(good, **settings)[name] for name, _ in capi.FrameHistorySettings._fields_])
        i = capi.FrameHistoryImages(*[dict(pointers, **images)[name] for name, _ in capi.FrameHistoryImages._fields_])
        before = bytes(history)
        flush_c_output()
        capfd.readouterr()
        assert lib.accumulate_frame_history(C.byref(history), C.byref(app), C.byref(s), C.byref(i)) == 1, (settings, images)
        flush_c_output()
        printed = capfd.readouterr().out
        assert printed.count("\n") == 1 and printed.endswith("\n") and len(printed) > 20, (settings, images, printed)
        assert bytes(history) == before
        return printed

    for settings in [dict(max_length=0.999), dict(max_length=-1.0), dict(max_length=nan), dict(max_length=inf), dict(sigma_depth=0.0), dict(sigma_depth=-1.0),
                     dict(sigma_depth=nan), dict(sigma_depth=inf), dict(normal_threshold=1.001), dict(normal_threshold=-1.001), dict(normal_threshold=nan),
                     dict(normal_threshold=inf), dict(spatial_length=65), dict(spatial_length=0xFFFFFFFF)]:
        assert "largest length" in refused(settings, {})
    for images in [dict(colour=None), dict(position=None), dict(normal=None), dict(out_colour=None), dict(colour=0x10004), dict(position=0x20001),
                   dict(normal=0x3000C), dict(reprojection=0x40008), dict(modulation=0x50002), dict(out_colour=0x60004), dict(out_variance=0x70008)]:
        assert "16-byte aligned" in refused({}, images)
    # nothing wrong but the history, which was never created
    assert "create_frame_history" in refused({}, {})
    assert "create_frame_history" in refused(dict(max_length=1.0, normal_threshold=-1.0, spatial_length=0), dict(reprojection=None, modulation=None, out_variance=None))
    half_made = capi.FrameHistory.from_buffer_copy(bytes(made_up))
    half_made.normal[1] = None
    assert "create_frame_history" in refused({}, {}, half_made)
    # overlaps
    for name in ("colour", "position", "normal", "reprojection", "modulation"):
        assert "overlaps" in refused({}, dict(out_colour=pointers[name]), made_up)
        assert "overlaps" in refused({}, dict(out_variance=pointers[name] + image_bytes - 16), made_up)
        assert "overlaps" in refused({}, dict(out_variance=pointers[name] - image_bytes + 16), made_up)
    assert "overlaps" in refused({}, dict(out_variance=pointers["out_colour"]), made_up)
    assert "overlaps" in refused({}, dict(out_variance=pointers["out_colour"] + image_bytes - 16), made_up)
    for key in frame_history.HISTORY_IMAGES:
        for j in range(2):
            assert "overlaps" in refused({}, dict(out_colour=getattr(made_up, key)[j]), made_up)
            assert "overlaps" in refused({}, dict(out_variance=getattr(made_up, key)[j] + image_bytes - 16), made_up)
    # an extent that is none
    created = capi.FrameHistory()
    for width, height in ((0, 0), (0, 5), (5, 0), (capi.FRAME_HISTORY_MAX_EXTENT + 1, 4), (4, 0xFFFFFFFF)):
        flush_c_output()
        capfd.readouterr()
        assert lib.create_frame_history(C.byref(created), C.byref(app), width, height) == 1
        flush_c_output()
        assert capfd.readouterr().out.count("\n") == 1
        assert not created.accumulated and not created.colour[0]
    # reset: the counter and nothing else
    made_up.frame_count, made_up.current = 7, 1
    before = bytes(made_up)
    lib.reset_frame_history(C.byref(made_up))
    assert made_up.frame_count == 0 and made_up.current == 1
    made_up.frame_count = 7
    assert bytes(made_up) == before
    with pytest.raises(ValueError):
        frame_history.check_settings(dict(max_length=0.5))
    with pytest.raises(ValueError):
        frame_history.check_settings(dict(normal_threshold=nan))
    with pytest.raises(ValueError):
        frame_history.check_settings(dict(spatial_length=65))
