"""Light shafts, kept verdicts (csrc/light_shafts.h, "Verdicts that are still true"): a frame context keeps a byte copy of
everything the verdicts of its last launch were derived from - launch geometry, tree, visibility buffer, camera, every
light's record - and while the arrangement and a light are byte-equal to that copy, the pair's "clear", its occluder list,
"no shaft" and "no shaded pixel" are kept instead of walked again.  A kept verdict is the verdict, so every frame must be
the frame of a renderer that walks every pair in every frame (VKR_SHAFT_REST=0, the cold path), in every bit: no
tolerance anywhere, a single differing word fails.

Every test renders a sequence of frames twice, warm (the default) and cold, and compares frame by frame."""
import numpy as np
import pytest

from vulkan_renderer_amd import renderer, synthetic

pytestmark = pytest.mark.gpu

CLEAR, LIST, NO_PIXELS, GEOMETRY, TOO_LONG, QUEUE_FULL, TRIANGLE, RESTING = 1, 2, 16, 17, 18, 19, 20, 21
KEPT_KINDS = (CLEAR, LIST, NO_PIXELS, GEOMETRY)


@pytest.fixture(scope="module")
def large_dataset(tmp_path_factory):
    return synthetic.write_dataset(str(tmp_path_factory.mktemp("reuse_large")), seed=4321, ltc_resolution=32, fresnel_count=16, large={})


@pytest.fixture(params=["benchmark", "large"])
def scene(request, big_dataset, large_dataset):
    return request.param, (big_dataset if request.param == "benchmark" else large_dataset)


def start(dataset, frames_in_flight, config=3, width=960, height=544, **kw):
    r = renderer.Renderer(frames_in_flight=frames_in_flight, **kw)
    renderer.setup_config(r, config, dataset, width=width, height=height, acceleration_structure="sah_device")
    r.create_targets()
    return r


def frame_of(r, words=False):
    out = {"image": r.read_radiance(), "rays": r.last_ray_count(), "stats": r.light_shaft_statistics()}
    if words:
        out["words"] = r.light_shaft_words()
    return out


def sequences(monkeypatch, begin, steps, words=False):
    """Renders one frame per entry of `steps` (a callable that changes the arrangement before the frame, or None), warm and
    then cold (VKR_SHAFT_REST=0), each time with a newly created pass - the frame pipeline with its contexts, tables and
    copies of the inputs lives and dies with the pass, and reads the environment when its first frame is rendered - on the
    scene that begin() has loaded -> ([frame_of()] warm, [frame_of()] cold).
    (One loaded scene for both, so that statistics can be compared exactly: how many walks give up as too long depends on the
    tree, and the first version of this file, with a renderer and a build of its own for the cold frames, once saw the first
    frames of the two differ in those counts while every pixel was equal.  Sequences whose steps change camera, lights or
    size set them in their first step, so that both start from the same arrangement.)"""
    r = begin()
    out = []
    try:
        for cold in (False, True):
            if cold:
                monkeypatch.setenv("VKR_SHAFT_REST", "0")
            else:
                monkeypatch.delenv("VKR_SHAFT_REST", raising=False)
            r.sync()
            r.create_pass()
            r.render_visibility()
            frames = []
            for step in steps:
                if step is not None:
                    step(r)
                r.render()
                frames.append(frame_of(r, words and not cold))
            out.append(frames)
    finally:
        r.close()
        monkeypatch.delenv("VKR_SHAFT_REST", raising=False)
    return out


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_frames_equal(warm, cold):
    assert len(warm) == len(cold)
    for index, (w, c) in enumerate(zip(warm, cold)):
        assert same_bits(w["image"], c["image"]), (index, int((w["image"].view(np.uint32) != c["image"].view(np.uint32)).any(axis=-1).sum()))


def decided(stats):
    return stats["clear_pairs"] + stats["list_pairs"]


@pytest.mark.parametrize("frames_in_flight", [1, 3])
def test_standing_still(scene, monkeypatch, frames_in_flight):
    """4 x depth frames of one arrangement: every frame is the cold frame; from a context's second frame on the pairs that
    need no tracing never fall below the first frame's, and the ray count never rises."""
    name, dataset = scene
    depth = frames_in_flight
    begin = lambda: start(dataset, frames_in_flight)
    warm, cold = sequences(monkeypatch, begin, [None] * (4 * depth), words=True)
    assert_frames_equal(warm, cold)
    first = warm[0]
    print(name, first["stats"], [f["rays"] for f in warm])
    assert decided(first["stats"]) > 0
    for index, frame in enumerate(warm):
        stats = frame["stats"]
        assert stats["pairs"] == first["stats"]["pairs"] == decided(stats) + sum(stats["not_clear"].values())
        if index < depth:
            # a context's first frame is cold: the cold renderer's statistics exactly
            assert stats == cold[index]["stats"] and frame["rays"] == cold[index]["rays"], index
        else:
            assert decided(stats) >= decided(first["stats"]), (index, stats)
            assert frame["rays"] <= first["rays"], (index, frame["rays"], first["rays"])
            # what was decided without tracing (or has no shaft, or no pixel) in the context's frame before is word for word there
            before, now = warm[index - depth]["words"], frame["words"]
            keep = np.isin(before & 0xFF, KEPT_KINDS)
            assert np.array_equal(now[keep], before[keep]), index


def moved(lights, which, offset):
    out = [dict(l) for l in lights]
    t = out[which]["translation"]
    out[which]["translation"] = (t[0] + offset[0], t[1] + offset[1], t[2] + offset[2])
    return out


@pytest.mark.parametrize("frames_in_flight", [1, 3])
def test_one_of_four_lights_moves(scene, monkeypatch, frames_in_flight):
    """Light 2 moves before every frame, the others stay: frames equal the cold ones, and what the three fixed lights had
    as clear / list / no shaft / no pixel in a context's previous frame is there word for word.  Resting words age and
    walks that were too long are repeated, as they always were."""
    name, dataset = scene
    depth = frames_in_flight
    lights = synthetic.config_lights(3)
    moving = 2
    steps = [(lambda r, k=k: r.set_lights(moved(lights, moving, (0.03 * k, -0.02 * k, 0.01 * k)))) for k in range(4 * depth)]
    begin = lambda: start(dataset, frames_in_flight)
    warm, cold = sequences(monkeypatch, begin, steps, words=True)
    assert_frames_equal(warm, cold)
    fixed = [i for i in range(len(lights)) if i != moving]
    for index in range(depth, len(warm)):
        before, now = warm[index - depth]["words"], warm[index]["words"]
        assert before.shape == now.shape
        kind_before, kind_now = before & 0xFF, now & 0xFF
        for light in fixed:
            keep = np.isin(kind_before[:, light], KEPT_KINDS)
            assert keep.any()
            assert np.array_equal(now[keep, light], before[keep, light]), (index, light)
            # resting words age by one frame or are walked again
            rested = (kind_before[:, light] == RESTING) & (kind_now[:, light] == RESTING)
            assert np.array_equal((now[rested, light] >> 8) & 0xFF, ((before[rested, light] >> 8) & 0xFF) + 1), (index, light)
            failed = kind_before[:, light] == TRIANGLE
            assert (kind_now[failed, light] == RESTING).all() and (((now[failed, light] >> 8) & 0xFF) == 1).all(), (index, light)
            # a walk that was too long (or filled its queue) is repeated: never kept, never resting
            again = np.isin(kind_before[:, light], (TOO_LONG, QUEUE_FULL))
            assert not (kind_now[again, light] == RESTING).any(), (index, light)
        # the moved light leans on nothing: no word of it rests (its record differs from the one its verdicts came from)
        assert not (kind_now[:, moving] == RESTING).any(), index
        # a patch without a shaded pixel stays one, whatever the lights do
        assert np.array_equal(kind_now == NO_PIXELS, kind_before == NO_PIXELS), index


@pytest.mark.parametrize("frames_in_flight", [1, 3])
def test_a_light_that_moves_and_comes_back(scene, monkeypatch, frames_in_flight):
    """A, B, A (each for one frame per context): A's second visit must not lean on A's first - the context's previous
    launch was B, and its table and lists hold B's verdicts."""
    name, dataset = scene
    depth = frames_in_flight
    a = synthetic.config_lights(3)
    b = moved(a, 1, (0.8, -0.6, 0.4))
    steps = []
    for lights in (a, b, a, b, a):
        steps += [lambda r, lights=lights: r.set_lights(lights)] * depth
    begin = lambda: start(dataset, frames_in_flight)
    warm, cold = sequences(monkeypatch, begin, steps, words=True)
    assert_frames_equal(warm, cold)
    for index in range(depth, len(warm)):
        # light 1 differs from the context's frame before in every frame: none of its pairs rests
        assert not ((warm[index]["words"][:, 1] & 0xFF) == RESTING).any(), index


@pytest.mark.parametrize("frames_in_flight", [1, 3])
def test_the_camera_moves(scene, monkeypatch, frames_in_flight):
    """Every verdict is stale after a camera move: nothing may be kept, nothing may rest - frames AND statistics are the
    cold renderer's exactly."""
    name, dataset = scene
    cam = synthetic.DEFAULT_CAMERA

    def nudge(k):
        def step(r):
            position = (cam["position"][0] + 0.01 * k, cam["position"][1] - 0.005 * k, cam["position"][2])
            r.set_camera(position, cam["rotation_x"], cam["rotation_z"] + 0.002 * k, cam["vertical_fov"], cam["near"], cam["far"])
            # (the visibility buffer belongs to the camera)
            r.render_visibility()
        return step
    steps = [nudge(k) for k in range(3 * frames_in_flight + 1)]
    begin = lambda: start(dataset, frames_in_flight)
    warm, cold = sequences(monkeypatch, begin, steps)
    assert_frames_equal(warm, cold)
    for index, (w, c) in enumerate(zip(warm, cold)):
        assert w["stats"] == c["stats"] and w["rays"] == c["rays"], (index, w["stats"], c["stats"])


@pytest.mark.parametrize("frames_in_flight", [1, 3])
def test_the_camera_moves_under_the_same_visibility_buffer(big_dataset, monkeypatch, frames_in_flight):
    """set_camera alone (the visibility buffer keeps the first camera's primitives, as for a caller that rasterises
    elsewhere and is a frame late): the camera's bytes are part of the arrangement by themselves"""
    cam = synthetic.DEFAULT_CAMERA
    def nudge(k):
        def step(r):
            r.set_camera((cam["position"][0] + 1.0e-4 * k, cam["position"][1], cam["position"][2]), cam["rotation_x"], cam["rotation_z"], cam["vertical_fov"], cam["near"], cam["far"])
            if k == 0:
                r.render_visibility()
        return step
    steps = [nudge(k) for k in range(3 * frames_in_flight + 1)]
    begin = lambda: start(big_dataset, frames_in_flight)
    warm, cold = sequences(monkeypatch, begin, steps)
    assert_frames_equal(warm, cold)
    for index, (w, c) in enumerate(zip(warm, cold)):
        assert w["stats"] == c["stats"] and w["rays"] == c["rays"], (index, w["stats"], c["stats"])


@pytest.mark.parametrize("how", ["render_visibility", "mark_inputs_changed", "upload_visibility"])
@pytest.mark.parametrize("frames_in_flight", [1, 3])
def test_inputs_changed_behind_the_same_bytes(scene, monkeypatch, frames_in_flight, how):
    """The visibility buffer is rewritten (with what it held, but the pass cannot know): everything is dropped for one
    frame per context - those frames have the cold statistics - and kept again afterwards."""
    name, dataset = scene
    depth = frames_in_flight

    def rewrite(r):
        if how == "render_visibility":
            r.render_visibility()
        elif how == "upload_visibility":
            r.upload_visibility(r.read_visibility())
        else:
            r.mark_inputs_changed()
    steps = [None] * (2 * depth) + [rewrite] + [None] * (2 * depth - 1)
    begin = lambda: start(dataset, frames_in_flight)
    warm, cold = sequences(monkeypatch, begin, steps, words=True)
    assert_frames_equal(warm, cold)
    for index in list(range(depth)) + list(range(2 * depth, 3 * depth)):
        assert warm[index]["stats"] == cold[index]["stats"] and warm[index]["rays"] == cold[index]["rays"], (index, warm[index]["stats"])
    if name == "large":
        # (the scene where pairs rest: a frame that leans on the one before shows it)
        for index in list(range(depth, 2 * depth)) + list(range(3 * depth, 4 * depth)):
            assert warm[index]["stats"]["not_clear"]["other"] > 0, index


@pytest.mark.parametrize("frames_in_flight", [1, 3])
def test_the_buffers_grow(scene, monkeypatch, frames_in_flight):
    """small, larger, small again in one renderer: tables and lists are allocated anew for the larger frame (and hold
    nothing of the small one), and the small frame afterwards finds the larger frame's words in them"""
    name, dataset = scene
    depth = frames_in_flight

    def resize(width, height):
        def step(r):
            r.sync()
            r.set_settings(width=width, height=height)
            r.create_targets()
            r.render_visibility()
        return step
    steps = [None] * (2 * depth) + [resize(1280, 720)] + [None] * (2 * depth - 1) + [resize(640, 368)] + [None] * (2 * depth - 1)
    begin = lambda: start(dataset, frames_in_flight, width=640, height=368)
    warm, cold = sequences(monkeypatch, begin, steps)
    assert_frames_equal(warm, cold)
    for first in (0, 2 * depth, 4 * depth):
        for index in range(first, first + depth):
            assert warm[index]["stats"] == cold[index]["stats"] and warm[index]["rays"] == cold[index]["rays"], (index, warm[index]["stats"])
        for index in range(first + depth, first + 2 * depth):
            assert decided(warm[index]["stats"]) >= decided(warm[first]["stats"]) and warm[index]["rays"] <= warm[first]["rays"], index


@pytest.mark.parametrize("frames_in_flight", [1, 2, 3])
def test_config_4_in_three_bands(big_dataset, monkeypatch, frames_in_flight):
    """Config 4 at 1920x1080 as three launches per frame: a band's geometry is part of the arrangement, so a context keeps
    verdicts only when it meets the same band again (three bands on three contexts, or on one: always; on two: never).
    Equal frames whatever band lands on whatever context.
    (The bands are forced through the pass's band_count: a budget in VKR_WAVEFRONT_BUDGET_MIB cannot split a 1920x1080
    frame, whose 8 160 blocks are less than two bands of the smallest size that plan_bands() makes by itself.)"""
    begin = lambda: start(big_dataset, frames_in_flight, config=4, width=1920, height=1080, band_count=3)

    def check_bands(r):
        assert r.app.shading_pass.last_band_count in (0, 3)
    steps = [check_bands] * 7
    warm, cold = sequences(monkeypatch, begin, steps)
    assert_frames_equal(warm, cold)
    for index, frame in enumerate(warm):
        assert frame["rays"] <= warm[0]["rays"], index


def test_fast_arithmetic_mode(big_dataset, monkeypatch):
    begin = lambda: start(big_dataset, 2, width=1280, height=720, arithmetic="fast")
    warm, cold = sequences(monkeypatch, begin, [None] * 6)
    assert_frames_equal(warm, cold)
    assert decided(warm[-1]["stats"]) >= decided(warm[0]["stats"]) > 0 and warm[-1]["rays"] <= warm[0]["rays"]
