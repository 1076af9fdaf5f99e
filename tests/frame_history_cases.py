"""Synthetic inputs of the frame history (include/vkr_frame_history.h), shared by tests/test_frame_history.py (CPU: the
numpy restatement against independent statements, and the conditions that make each sequence mean something) and
tests/test_gpu_frame_history.py (the kernels against the restatement).  Not collected by pytest.

A sequence is six frames on valley() of tests/frame_filter_cases.py: its position, normal and modulation, and a colour per
frame that is the valley's noise-free colour times a factor per pixel and frame out of [0.6, 1.4) (times the modulation, as
a renderer hands it over).  The geometry stands still in the image unless the sequence says otherwise; the reprojection
image claims where each pixel was, and the rule takes its word within its guards: taps that land across the crease fail the
normal test, taps across the depth step the plane test, taps in the uncovered rectangle are uncovered."""
import functools

import numpy as np

import frame_filter_cases as filter_cases
from vulkan_renderer_amd import frame_history

f32 = np.float32
FRAME_COUNT = 6
SETTINGS = dict(max_length=32.0, sigma_depth=0.02, normal_threshold=0.9, spatial_length=4)
IMAGE_NAMES = ("colour", "position", "normal", "reprojection", "modulation")


def shift_image(width, height, dx, dy):
    """What render_feature_buffers() writes for a camera under which pixel (x, y) was at (x + dx, y + dy): the flag is 1 where
    that is in the frame by the rule of include/vkr_feature_buffers.h"""
    ys, xs = np.mgrid[0:height, 0:width]
    X, Y = (xs + dx).astype(f32), (ys + dy).astype(f32)
    inside = (X >= -0.5) & (X < width - 0.5) & (Y >= -0.5) & (Y < height - 0.5)
    return np.stack([X, Y, np.full((height, width), 2.5, f32), inside.astype(f32)], axis=-1).astype(f32)


def frame_colour(images, rng):
    colour = images["clean"].copy()
    colour[..., :3] *= rng.uniform(0.6, 1.4, colour.shape[:2] + (1,)).astype(f32)
    if images["modulation"] is not None:
        colour[..., :3] *= np.maximum(images["modulation"][..., :3], f32(1.0 / 256.0))
    return colour


def crop(images, x0, width):
    return {name: (value[:, x0:x0 + width].copy() if isinstance(value, np.ndarray) else value) for name, value in images.items()}


def lies(width, height):
    """The identity with pixels that must not be believed (flag 1, X of 1e30, NaN, -5 and `width`: no history, and no load
    from where they point), a column whose flag is 0, a row whose flag is 2, and the corner (width - 1, 0) at (x + 15 / 16,
    y - 15 / 16): three taps out of the frame, the fourth with weight 1 / 256 < 1 / 64"""
    r = shift_image(width, height, 0, 0)
    liars = {}
    if width >= 16 and height >= 16:
        y = height // 2 - 2
        for i, value in enumerate((1.0e30, np.nan, -5.0, float(width), -np.inf, 4.0e9)):
            liars[(y, 5 + 2 * i)] = value
            r[y, 5 + 2 * i, 0] = value
        for i, value in enumerate((1.0e30, np.nan, -1.5, float(height), -3.0e9)):
            liars[(y + 2, 5 + 2 * i)] = value
            r[y + 2, 5 + 2 * i, 1] = value
        r[:, width // 2 + 3, 3] = 0.0
        r[height - 2, :, 3] = 2.0
    r[0, width - 1, :2] = (width - 1 + 15.0 / 16.0, -15.0 / 16.0)
    return r, liars


# name -> (width, height, what build() reads)
SEQUENCES = {
    "whole": (83, 45, dict(seed=11, shift=(3, -2))),
    "fraction": (83, 45, dict(seed=12, shift=(2.25, -1.5), modulation=True)),
    "still_null": (83, 45, dict(seed=13)),
    "still_identity": (83, 45, dict(seed=13, shift=(0, 0))),
    "moving": (83, 45, dict(seed=14, moving=True)),
    "non_finite": (83, 45, dict(seed=15, non_finite=True, modulation=True)),
    "lying": (83, 45, dict(seed=16, lying=True)),
    "saturating": (16, 16, dict(seed=17, modulation=True, settings=dict(max_length=4.0))),
    "no_spatial": (33, 35, dict(seed=18, shift=(2.25, -1.5), settings=dict(spatial_length=0))),
    "33x35": (33, 35, dict(seed=19, shift=(-1.75, 0.5), modulation=True)),
    "7x3": (7, 3, dict(seed=20, shift=(0.5, 0.25))),
    # (the valley of one pixel is not covered: these are the covered pixel (3, 0) of a 7x3 valley)
    "1x1": (1, 1, dict(seed=21, window=(7, 3, 3, 0))),
    "1x1_modulated": (1, 1, dict(seed=22, modulation=True, shift=(-0.5, 0.25), window=(7, 3, 3, 0))),
}
# (frame, what the colour gets) of the sequence with colours that are not finite: the first frame has no history
NON_FINITE_FRAMES = {0: "first", 3: "later"}


def settings(name):
    return dict(SETTINGS, **SEQUENCES[name][2].get("settings", {}))


@functools.lru_cache(maxsize=None)
def build(name):
    """-> list of FRAME_COUNT dicts of read-only float32 images (height, width, 4) per IMAGE_NAMES; reprojection and
    modulation may be None"""
    width, height, spec = SEQUENCES[name]
    rng = np.random.default_rng(1000 + spec["seed"])
    moving = spec.get("moving", False)
    # (moving: the valley slides one pixel per frame along x under a camera that is said to stand still.  Its two planes
    # slide along themselves, so only the depth step, the crease, the uncovered rectangle and the special pixels move against
    # what was there: pixels are uncovered, covered again, and fail the plane and the normal test at the edges.)
    base_width, base_height, x0, y0 = spec.get("window", (width + (FRAME_COUNT - 1 if moving else 0), height, 0, 0))
    base = filter_cases.valley(base_width, base_height, seed=spec["seed"], variance=None, modulation=spec.get("modulation", False))
    if "window" in spec:
        base = {key: (value[y0:y0 + height].copy() if isinstance(value, np.ndarray) else value) for key, value in crop(base, x0, width).items()}
    reprojection = None
    if "shift" in spec:
        reprojection = shift_image(width, height, *spec["shift"])
    if spec.get("lying"):
        reprojection = lies(width, height)[0]
    frames = []
    for index in range(FRAME_COUNT):
        images = crop(base, index, width) if moving else base
        colour = frame_colour(images, rng)
        if spec.get("non_finite") and index in NON_FINITE_FRAMES:
            covered = np.argwhere(images["position"][..., 3] > 0)
            chosen = covered[rng.choice(len(covered), 6, replace=False)]
            for i, (y, x) in enumerate(chosen):
                colour[y, x, i % 3] = (np.nan, np.inf, -np.inf)[i % 3]
                if i == 5:
                    colour[y, x, :3] = np.nan
        frame = dict(colour=colour, position=images["position"], normal=images["normal"], reprojection=reprojection, modulation=images["modulation"])
        for value in frame.values():
            if value is not None:
                value.setflags(write=False)
        frames.append(frame)
    return frames


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> list per frame of (state, out_colour, out_variance, diagnostics) of the numpy restatement; computed once, left
    unchanged"""
    width, height, _ = SEQUENCES[name]
    state, results = frame_history.new_state(width, height), []
    for frame in build(name):
        diagnostics = {}
        state, out_colour, out_variance = frame_history.accumulate(state, frame["colour"], frame["position"], frame["normal"], frame["reprojection"],
                                                                   frame["modulation"], settings(name), diagnostics)
        for image in [out_colour, out_variance] + [state[key] for key in frame_history.HISTORY_IMAGES]:
            image.setflags(write=False)
        results.append((state, out_colour, out_variance, diagnostics))
    return results


def assert_conditions(name):
    """What the sequence is there for, on the numpy side"""
    width, height, spec = SEQUENCES[name]
    frames, results = build(name), expected(name)
    assert len(frames) == len(results) == FRAME_COUNT
    first = results[0][3]
    # the first frame finds no history
    assert first["no_history"] == first["covered"] == first["not_usable"] and sum(first[reason] for reason in frame_history.TAP_REJECTIONS) == 0
    for (state, out_colour, out_variance, diagnostics), frame in zip(results, frames):
        covered = frame["position"][..., 3] > 0
        assert diagnostics["covered"] == int(covered.sum())
        assert out_colour[..., 3].tobytes() == frame["colour"][..., 3].tobytes() and out_colour[~covered].tobytes() == frame["colour"][~covered].tobytes()
        assert not state["colour"][~covered].any() and not state["moments"][~covered].any() and not out_variance[~covered].any()
        assert state["position"].tobytes() == frame["position"].tobytes() and state["normal"].tobytes() == frame["normal"].tobytes()
        # nothing that is not finite is ever kept
        assert np.isfinite(state["colour"]).all() and np.isfinite(state["moments"]).all() and (out_variance[covered][:, 3] == 1).all()
        assert (out_variance[..., :3] >= 0).all() and not state["moments"][..., 3].any()
    if (width, height) == (83, 45):
        assert width > 64 and height > 32 and width % 16 and height % 16 and covered.sum() > 1000 and (~covered).sum() > 100
        # the spatial estimate is taken in the first frame, by every covered pixel
        assert first["spatial"] == first["covered"] - first["skipped_without_history"] > 0
    later = [diagnostics for _, _, _, diagnostics in results[1:]]
    if name == "whole":
        # b = 1, 0, 0, 0: three taps without weight per pixel, the history of the shifted pixel or none
        for diagnostics in later:
            usable = diagnostics["covered"] - diagnostics["not_usable"]
            assert diagnostics["weight"] + diagnostics["frame"] >= 3 * usable and diagnostics["weight"] > 2 * usable and diagnostics["not_usable"] > 0
            assert diagnostics["uncovered"] > 0 and diagnostics["plane"] > 0 and diagnostics["normal"] > 0
    if name == "fraction":
        assert frames[0]["modulation"] is not None
        for diagnostics in later:
            # (a pixel whose flag is 1 has X < width - 0.5: its right taps can leave the frame)
            assert diagnostics["weight"] == 0 and diagnostics["frame"] > 0 and diagnostics["uncovered"] > 0 and diagnostics["plane"] > 0 and diagnostics["normal"] > 0
            assert 0 < diagnostics["not_usable"] < diagnostics["no_history"] < diagnostics["covered"]
        # lengths that are no integers
        length = results[-1][0]["colour"][..., 3]
        assert (length != np.floor(length)).any()
    if name in ("still_null", "still_identity"):
        assert (frames[0]["reprojection"] is None) == (name == "still_null")
        for index, diagnostics in enumerate(later, 1):
            # (a tap out of the frame is counted as that, whatever its weight)
            assert diagnostics["no_history"] == 0 and diagnostics["weight"] + diagnostics["frame"] == 3 * diagnostics["covered"] and diagnostics["frame"] > 0
            assert diagnostics["uncovered"] == diagnostics["plane"] == diagnostics["normal"] == 0
            # n' = index + 1: below the spatial length in frames 1 ... spatial_length - 1, then by no pixel
            assert diagnostics["spatial"] == (diagnostics["covered"] if index + 1 < SETTINGS["spatial_length"] else 0), index
        assert FRAME_COUNT > SETTINGS["spatial_length"]
    if name == "moving":
        assert frames[0]["reprojection"] is None and frames[0]["position"].tobytes() != frames[1]["position"].tobytes()
        for index, diagnostics in enumerate(later, 1):
            before, now = frames[index - 1]["position"][..., 3] > 0, frames[index]["position"][..., 3] > 0
            assert (before & ~now).any() and (now & ~before).any()
            assert diagnostics["uncovered"] == int((now & ~before).sum()) and diagnostics["plane"] > 0 and diagnostics["normal"] > 0
            assert diagnostics["no_history"] == diagnostics["low_weight"] > 0 and diagnostics["spatial"] > 0
    if name == "non_finite":
        for index, (state, out_colour, out_variance, diagnostics) in enumerate(results):
            assert (diagnostics["skipped_sample"] == 6) == (index in NON_FINITE_FRAMES), index
            assert diagnostics["skipped_without_history"] == (6 if index == 0 else 0)
        # without history: length 0, black; the next frame starts there
        bad = ~np.isfinite(frames[0]["colour"][..., :3]).all(axis=-1)
        assert not results[0][0]["colour"][bad].any() and (results[1][0]["colour"][bad][:, 3] == 1).all()
    if name == "lying":
        r, liars = lies(width, height)
        assert len(liars) == 11 and (r[..., 3] == 0).sum() >= height - 1 and (r[..., 3] == 2).sum() > 0
        covered = frames[0]["position"][..., 3] > 0
        for index in range(1, FRAME_COUNT):
            length = results[index][0]["colour"][..., 3]
            for (y, x) in liars:
                assert covered[y, x] and length[y, x] == 1, (y, x)
            assert length[0, width - 1] == 1 and covered[0, width - 1] and results[index][3]["low_weight"] == 1
            assert results[index][3]["not_usable"] > height
            believed = covered & (r[..., 3] == 1) & (r[..., 0] == np.floor(r[..., 0])) & (r[..., 0] >= 0) & (r[..., 0] < width) & (r[..., 1] >= 0) & (r[..., 1] < height)
            assert (length[believed] == index + 1).all()
    if name == "saturating":
        lengths = [float(state["colour"][..., 3].max()) for state, _, _, _ in results]
        assert lengths == [1.0, 2.0, 3.0, 4.0, 4.0, 4.0] and settings(name)["max_length"] == 4.0
    if name == "no_spatial":
        assert all(diagnostics["spatial"] == 0 for _, _, _, diagnostics in results) and settings(name)["spatial_length"] == 0
    if name.startswith("1x1"):
        # three of the four taps are out of the frame; the fourth has weight 1, or 3 / 8 under the shift by a fraction
        assert all(diagnostics["covered"] == 1 and diagnostics["frame"] == 3 and diagnostics["no_history"] == 0 for diagnostics in later)
        assert results[-1][0]["colour"][0, 0, 3] == FRAME_COUNT
    if name == "7x3":
        assert width < 7 + 1 and height < 7 and all(diagnostics["spatial"] > 0 for _, _, _, diagnostics in results[:2])


def assert_every_reason_and_class_occurs():
    """Over the 83x45 sequences: every reason to reject a tap, every class of pixels"""
    totals = dict.fromkeys(frame_history.TAP_REJECTIONS + frame_history.PIXEL_CLASSES, 0)
    for name, (width, height, _) in SEQUENCES.items():
        if (width, height) == (83, 45):
            for _, _, _, diagnostics in expected(name):
                for key in totals:
                    totals[key] += diagnostics[key]
    assert all(total > 0 for total in totals.values()), totals
    return totals
