"""Inputs of accumulate_moving_frame_history() (include/vkr_frame_history.h, "Moving geometry"), shared by
tests/test_frame_history_motion.py (CPU: the changed tap test of the numpy restatement) and
tests/test_gpu_frame_history_motion.py (the kernels against it).  Not collected by pytest.

The translating valley: six frames on valley() of tests/frame_filter_cases.py, whose positions (x, y) -> (X, Y, Z) are those
of a camera that looks along z without perspective.  The whole valley moves by STEP along z per frame - along the mean of its
two normals -, so every surface point stays at its pixel: the reprojection is the identity, and previous_position holds the
previous frame's position of the same pixel.  STEP is far more than sigma_depth times any distance in the frame: the rule
without previous_position rejects every tap.

The sequences of tests/frame_history_cases.py get a previous_position image too: this frame's position pushed along the
pixel's normal by up to two plane thresholds either way, so that about half of the taps that passed the plane test fail it
and some that failed it pass."""
import functools

import numpy as np

import frame_filter_cases as filter_cases
import frame_history_cases as history_cases
from vulkan_renderer_amd import frame_history

f32 = np.float32
FRAME_COUNT = history_cases.FRAME_COUNT
SETTINGS = history_cases.SETTINGS
STEP = f32(1.0)
# name -> (width, height, seed)
VALLEYS = {"valley_83x45": (83, 45, 31), "valley_33x35": (33, 35, 32), "valley_16x16": (16, 16, 33), "valley_7x3": (7, 3, 34)}


def as_previous(position, covered):
    """What render_motion_buffers() writes: {Q.xyz, 1} at covered pixels, sixteen zero bytes elsewhere"""
    out = np.zeros(position.shape, f32)
    out[covered, :3] = position[covered, :3]
    out[covered, 3] = 1.0
    return out


@functools.lru_cache(maxsize=None)
def valley(name):
    """-> list of FRAME_COUNT dicts of read-only float32 images: colour, position, normal, reprojection, modulation (None)
    and previous_position"""
    width, height, seed = VALLEYS[name]
    rng = np.random.default_rng(2000 + seed)
    base = filter_cases.valley(width, height, seed=seed, variance=None)
    covered = base["position"][..., 3] > 0
    reprojection = history_cases.shift_image(width, height, 0, 0)
    frames, before = [], None
    for index in range(FRAME_COUNT):
        position = base["position"].copy()
        X, Y, Z = position[..., 0], position[..., 1], position[..., 2] + f32(index) * STEP
        position[covered, 2] = Z[covered]
        position[covered, 3] = np.sqrt((X * X + Y * Y) + Z * Z)[covered]
        frame = dict(colour=history_cases.frame_colour(base, rng), position=position, normal=base["normal"], reprojection=reprojection, modulation=None,
                     previous_position=as_previous(position if before is None else before, covered))
        for value in frame.values():
            if value is not None:
                value.setflags(write=False)
        frames.append(frame)
        before = position
    return frames


@functools.lru_cache(maxsize=None)
def pushed(name):
    """-> list of FRAME_COUNT previous_position images for sequence `name` of tests/frame_history_cases.py"""
    rng = np.random.default_rng(3000 + history_cases.SEQUENCES[name][2]["seed"])
    sigma_depth = f32(history_cases.settings(name)["sigma_depth"])
    images = []
    for frame in history_cases.build(name):
        position, normal = frame["position"], frame["normal"]
        covered = position[..., 3] > 0
        with np.errstate(all="ignore"):
            push = rng.uniform(-2.0, 2.0, position.shape[:2]).astype(f32) * (sigma_depth * position[..., 3])
            moved = position.copy()
            moved[..., :3] = position[..., :3] + normal[..., :3] * push[..., None]
        image = as_previous(moved, covered)
        image.setflags(write=False)
        images.append(image)
    return images


def frames_of(name):
    """The frames of a valley, or of a sequence of tests/frame_history_cases.py with its pushed previous positions"""
    if name in VALLEYS:
        return valley(name)
    return [dict(frame, previous_position=previous) for frame, previous in zip(history_cases.build(name), pushed(name))]


def settings(name):
    return dict(SETTINGS) if name in VALLEYS else history_cases.settings(name)


def extent(name):
    return VALLEYS[name][:2] if name in VALLEYS else history_cases.SEQUENCES[name][:2]


NAMES = list(VALLEYS) + list(history_cases.SEQUENCES)


@functools.lru_cache(maxsize=None)
def expected(name, moving=True):
    """-> list per frame of (state, out_colour, out_variance, diagnostics) of the numpy restatement, with the frames'
    previous_position or, moving=False, without; computed once, left unchanged"""
    width, height = extent(name)
    state, results = frame_history.new_state(width, height), []
    for frame in frames_of(name):
        diagnostics = {}
        state, out_colour, out_variance = frame_history.accumulate(state, frame["colour"], frame["position"], frame["normal"], frame["reprojection"], frame["modulation"],
                                                                   settings(name), diagnostics, frame["previous_position"] if moving else None)
        for image in [out_colour, out_variance] + [state[key] for key in frame_history.HISTORY_IMAGES]:
            image.setflags(write=False)
        results.append((state, out_colour, out_variance, diagnostics))
    return results


def assert_valley_conditions(name):
    """What a translating valley is there for, from the case itself"""
    frames = valley(name)
    width, height, _ = VALLEYS[name]
    sigma_depth = f32(SETTINGS["sigma_depth"])
    covered = frames[0]["position"][..., 3] > 0
    assert covered.any() and frames[0]["previous_position"][covered][:, :3].tobytes() == frames[0]["position"][covered][:, :3].tobytes()
    ys, xs = np.mgrid[0:height, 0:width]
    for index in range(1, FRAME_COUNT):
        frame, before = frames[index], frames[index - 1]
        assert np.array_equal(frame["position"][..., 3] > 0, covered)
        # the reprojection says that every pixel stays, and previous_position is the previous frame's position there
        r = frame["reprojection"]
        assert np.array_equal(r[..., 0], xs) and np.array_equal(r[..., 1], ys) and (r[..., 3] == 1).all()
        assert frame["previous_position"][covered][:, :3].tobytes() == before["position"][covered][:, :3].tobytes()
        assert (frame["previous_position"][covered][:, 3] == 1).all() and not frame["previous_position"][~covered].any()
        # the motion: STEP along z, nothing else, and more than the plane test tolerates at every covered pixel
        d = (frame["position"][..., :3].astype(np.float64) - frame["previous_position"][..., :3])[covered]
        assert not d[:, :2].any() and (np.abs(d[:, 2] - float(STEP)) < 1.0e-6).all()
        along = np.abs((frame["normal"][..., :3].astype(np.float64)[covered] * d).sum(axis=-1))
        allowed = float(sigma_depth) * frame["position"][..., 3][covered]
        assert (along > 1.5 * allowed).all(), (index, float((along / allowed).min()))
