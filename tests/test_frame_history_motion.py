"""accumulate_moving_frame_history() (include/vkr_frame_history.h, "Moving geometry") without a GPU: what the numpy
restatement (vulkan_renderer_amd/frame_history.py) does with a valley that translates along its normal - without
previous_position every tap fails the plane test, with it the history grows frame by frame -, NULL previous_position, the
restatement against a plain loop in binary64, and the rejection diagnostics.  The cases: tests/frame_history_motion_cases.py."""
import numpy as np
import pytest

import frame_history_cases as history_cases
import frame_history_motion_cases as cases
from test_frame_history import U, loop_frame, loop_spatial
from vulkan_renderer_amd import frame_history

f32 = np.float32


@pytest.mark.parametrize("name", list(cases.VALLEYS))
def test_valleys_meet_their_conditions(name):
    cases.assert_valley_conditions(name)


@pytest.mark.parametrize("name", list(cases.VALLEYS))
def test_without_previous_position_a_translating_valley_never_finds_its_history(name):
    """What accumulate_frame_history() does with moving geometry: tap 0 of every covered pixel - the pixel itself, weight 1 -
    is rejected by the plane test, the other three have no weight or lie outside the frame; n' stays 1 in every frame"""
    frames, results = cases.frames_of(name), cases.expected(name, moving=False)
    covered = frames[0]["position"][..., 3] > 0
    for index, (state, out_colour, _, diagnostics) in enumerate(results):
        assert (state["colour"][..., 3][covered] == 1).all(), index
        assert out_colour[covered].tobytes() == frames[index]["colour"][covered].tobytes()
        if index:
            assert diagnostics["plane"] == diagnostics["covered"] == diagnostics["no_history"] == int(covered.sum()) and diagnostics["not_usable"] == 0
            assert diagnostics["normal"] == diagnostics["uncovered"] == 0 and diagnostics["weight"] + diagnostics["frame"] == 3 * diagnostics["covered"]


@pytest.mark.parametrize("name", list(cases.VALLEYS))
def test_with_previous_position_the_history_follows_the_valley(name):
    """n' is the frame number wherever the four taps are in the frame (and at the other covered pixels too: the taps out of
    the frame have no weight), and c' is the running mean within the bound of test_still_camera_gives_the_running_mean...:
    U |d| in d = c - c', 2 U |a d| in the product, U c' in the sum, the error of the frame before times 1 - a."""
    frames, results = cases.frames_of(name), cases.expected(name)
    width, height = cases.extent(name)
    covered = frames[0]["position"][..., 3] > 0
    ys, xs = np.mgrid[0:height, 0:width]
    four_taps = covered & (xs + 1 < width) & (ys + 1 < height)
    assert four_taps.any() and cases.FRAME_COUNT < cases.SETTINGS["max_length"]
    total, error, share = np.zeros((height, width, 3)), np.zeros((height, width, 3)), 0.0
    for index, (frame, (state, out_colour, _, diagnostics)) in enumerate(zip(frames, results)):
        c = frame["colour"][..., :3].astype(np.float64)
        a = 1.0 / (index + 1)
        previous_mean = total / max(index, 1)
        total += c
        mean = total / (index + 1)
        error = (1.0 - a) * error + 3.0 * U * a * np.abs(c - previous_mean) + U * mean if index else np.zeros_like(mean)
        assert (state["colour"][..., 3][four_taps] == index + 1).all() and (state["colour"][..., 3][covered] == index + 1).all(), index
        assert out_colour[..., :3].tobytes() == state["colour"][..., :3].tobytes() or not covered.all()
        difference = np.abs(out_colour[..., :3].astype(np.float64) - mean)[covered]
        allowed = 1.01 * error[covered] + 1.0e-30
        assert (difference <= allowed).all(), index
        if index:
            share = max(share, float((difference / allowed).max()))
            assert diagnostics["plane"] == diagnostics["normal"] == diagnostics["no_history"] == 0
    print("largest difference / bound: %.3f" % share)
    assert share > 1.0e-2


@pytest.mark.parametrize("name", ["valley_16x16", "fraction", "moving", "1x1_modulated"])
def test_null_previous_position_gives_the_bytes_of_accumulate(name):
    """previous_position=None is accumulate() as it was; an image that repeats this frame's positions changes no byte either"""
    state_a = state_b = state_c = frame_history.new_state(*cases.extent(name))
    for frame in cases.frames_of(name):
        arguments = (frame["colour"], frame["position"], frame["normal"], frame["reprojection"], frame["modulation"], cases.settings(name))
        a = frame_history.accumulate(state_a, *arguments)
        b = frame_history.accumulate(state_b, *arguments, previous_position=None)
        c = frame_history.accumulate(state_c, *arguments, previous_position=cases.as_previous(frame["position"], frame["position"][..., 3] > 0))
        for other in (b, c):
            assert a[1].tobytes() == other[1].tobytes() and a[2].tobytes() == other[2].tobytes()
            assert all(a[0][key].tobytes() == other[0][key].tobytes() for key in frame_history.HISTORY_IMAGES)
        state_a, state_b, state_c = a[0], b[0], c[0]
    if name not in cases.VALLEYS:
        assert [result[1].tobytes() for result in cases.expected(name, moving=False)] == [result[1].tobytes() for result in history_cases.expected(name)]
    with pytest.raises(ValueError):
        frame_history.accumulate(state_a, *arguments, previous_position=np.zeros((2, 2, 4), f32))


@pytest.mark.parametrize("name", ["valley_7x3", "valley_33x35", "7x3", "33x35", "saturating", "1x1_modulated"])
def test_restatement_equals_a_plain_loop_within_its_roundings(name):
    """The loop of tests/test_frame_history.py in binary64, frame by frame from the binary32 history of the restatement, and
    its bounds from the operation count.  The loop takes P_p from the frame's position: it is handed previous_position's xyz
    there, with this frame's distance - the one change of the rule; the spatial estimate keeps this frame's positions."""
    settings = frame_history.check_settings(cases.settings(name))
    state = frame_history.new_state(*cases.extent(name))
    worst, verdicts_differ = {}, False
    for index, frame in enumerate(cases.frames_of(name)):
        new_state, out_colour, out_variance = frame_history.accumulate(state, frame["colour"], frame["position"], frame["normal"], frame["reprojection"],
                                                                       frame["modulation"], settings, None, frame["previous_position"])
        was = frame["position"].copy()
        was[..., :3] = frame["previous_position"][..., :3]
        value, bound = loop_frame(state, dict(frame, position=was), settings)
        spatial_value, spatial_bound = loop_spatial(new_state, frame, settings)
        spatial = ~np.isnan(spatial_value[..., 0])
        got = {"c": new_state["colour"][..., :3], "s": new_state["moments"][..., :3], "n": new_state["colour"][..., 3:], "out_colour": out_colour[..., :3],
               "out_variance": out_variance[..., :3]}
        compare = ~np.isnan(value["c"][..., 0])
        assert compare.sum() > 0 and (compare == (frame["position"][..., 3] > 0)).all()
        for key in got:
            want, allowed = value[key], bound[key]
            if key == "out_variance":
                want, allowed = np.where(spatial[..., None], spatial_value, want), np.where(spatial[..., None], spatial_bound, allowed)
            difference = np.abs(got[key].astype(np.float64) - want)[compare]
            allowed = 1.01 * allowed[compare] + 1.0e-30
            worst[key] = max(worst.get(key, 0.0), float((difference / allowed).max()))
            assert (difference <= allowed).all(), (name, index, key, worst[key])
        still = frame_history.accumulate(state, frame["colour"], frame["position"], frame["normal"], frame["reprojection"], frame["modulation"], settings)
        verdicts_differ = verdicts_differ or still[0]["colour"].tobytes() != new_state["colour"].tobytes()
        state = new_state
    print(name, "largest difference / bound:", {key: round(share, 3) for key, share in worst.items()})
    assert max(worst.values()) > 1.0e-2
    # (the loop is told something that the rule without previous_position would not do)
    assert verdicts_differ


def test_rejection_diagnostics_name_every_reason_at_83x45():
    """Over the 83x45 sequences with their pushed previous positions: every reason to reject a tap and every class of pixels
    occurs, and the plane test decides differently than without previous_position"""
    totals = dict.fromkeys(frame_history.TAP_REJECTIONS + frame_history.PIXEL_CLASSES, 0)
    for name in history_cases.SEQUENCES:
        if cases.extent(name) != (83, 45):
            continue
        moving, still = cases.expected(name), cases.expected(name, moving=False)
        for (_, _, _, with_previous), (_, _, _, without) in zip(moving, still):
            for key in totals:
                totals[key] += with_previous[key]
            assert with_previous["covered"] == without["covered"] and with_previous["not_usable"] == without["not_usable"]
            assert with_previous["frame"] == without["frame"] and with_previous["weight"] == without["weight"]
        assert sum(d["plane"] for _, _, _, d in moving[1:]) > sum(d["plane"] for _, _, _, d in still[1:]), name
        # pushed by up to two thresholds: a good part of the taps still finds its surface
        assert sum(d["no_history"] for _, _, _, d in moving[1:]) < sum(d["covered"] for _, _, _, d in moving[1:]), name
    assert all(total > 0 for total in totals.values()), totals
