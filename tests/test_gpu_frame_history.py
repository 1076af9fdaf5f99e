"""The frame history (include/vkr_frame_history.h) on the device: every sequence of tests/frame_history_cases.py frame by
frame against the numpy restatement in every bit of both outputs (between guard bytes) and of the four history images, a
reset in the middle, the history behind rendered frames of a turning camera and in front of the frame filter, on the radiance
target between frames in flight, the three arithmetic modes of the pass, the refusals and the command line."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import frame_history_cases as cases
import png_cases
from helpers import GUARD_BYTE, Arena, DeviceBuffer, assert_same_bits, differing, flush_c_output, open_renderer
from vulkan_renderer_amd import capi, feature_buffers, frame_filter, frame_history, renderer

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def device():
    """A renderer with nothing but its device: the history needs no scene and no pass"""
    r = renderer.Renderer()
    yield r
    r.close()


class Uploads:
    """The images of a sequence on the device, each distinct array once"""

    def __init__(self):
        self.buffers = {}

    def images(self, frame, arena, want_variance=True):
        pointers = []
        for name in cases.IMAGE_NAMES:
            image = frame[name]
            if image is not None and id(image) not in self.buffers:
                self.buffers[id(image)] = (DeviceBuffer(max(image.nbytes, 16)), image)
                self.buffers[id(image)][0].upload(image)
            pointers.append(None if image is None else self.buffers[id(image)][0].ptr.value)
        return capi.FrameHistoryImages(*pointers, arena.address(0), arena.address(1) if want_variance else None)

    def free(self):
        for buffer, _ in self.buffers.values():
            buffer.free()


def settings_struct(values):
    return capi.FrameHistorySettings(float(values["max_length"]), float(values["sigma_depth"]), float(values["normal_threshold"]), int(values["spatial_length"]))


def assert_frame(history, arena, expected, want_variance, what):
    state, want_colour, want_variance_image, _ = expected
    got_colour, got_variance, guards_intact = arena.read()
    assert guards_intact, what
    assert_same_bits(got_colour, want_colour, what + ("out_colour",))
    if want_variance:
        assert_same_bits(got_variance, want_variance_image, what + ("out_variance",))
    else:
        assert (got_variance.view(np.uint8) == GUARD_BYTE).all(), what
    images = history.read()
    for key in frame_history.HISTORY_IMAGES:
        assert_same_bits(images[key], state[key], what + (key,))
    assert history.frame_count == state["frame_count"]


# ---- 1. the sequences against numpy --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(cases.SEQUENCES))
def test_sequences_equal_numpy_in_every_bit(device, name):
    """Frame by frame, two histories side by side: one with out_variance (and with it the second launch, unless the
    spatial length is 0), one without, whose variance image must stay untouched and whose other results are the same.  The
    kernels have no threshold in the extent: frames smaller than a workgroup's tile (7x3, 1x1), of exactly one (16x16) and of
    several with partial ones on both edges (83x45, 33x35) go the same way."""
    cases.assert_conditions(name)
    width, height, _ = cases.SEQUENCES[name]
    sequence, expected = cases.build(name), cases.expected(name)
    arena, uploads = Arena(width, height), Uploads()
    histories = {True: device.create_frame_history(width, height), False: device.create_frame_history(width, height)}
    lib = capi.load()
    try:
        settings = settings_struct(cases.settings(name))
        for index, frame in enumerate(sequence):
            for want_variance, history in histories.items():
                arena.reset()
                images = uploads.images(frame, arena, want_variance)
                assert lib.accumulate_frame_history(C.byref(history.history), C.byref(device.app), C.byref(settings), C.byref(images)) == 0
                assert_frame(history, arena, expected[index], want_variance, (name, index, want_variance))
    finally:
        for history in histories.values():
            history.close()
        uploads.free()
        arena.free()


def test_null_and_identity_reprojection_give_the_same_bytes():
    """(numpy's side of it; the device equals numpy in both sequences above)"""
    for a, b in zip(cases.expected("still_null"), cases.expected("still_identity")):
        assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
        assert all(a[0][key].tobytes() == b[0][key].tobytes() for key in frame_history.HISTORY_IMAGES)


def test_reset_in_the_middle_equals_a_fresh_history(device):
    name = "fraction"
    width, height, _ = cases.SEQUENCES[name]
    sequence, expected = cases.build(name), cases.expected(name)
    arena, uploads = Arena(width, height), Uploads()
    history = device.create_frame_history(width, height)
    lib = capi.load()
    try:
        settings = settings_struct(cases.settings(name))
        for index in (0, 1, 2, None, 0, 1, 2):
            if index is None:
                before = history.read()
                history.reset()
                assert history.frame_count == 0
                # (nothing but the counter: the images are as they were)
                assert all(before[key].tobytes() == history.read()[key].tobytes() for key in before)
                continue
            arena.reset()
            assert lib.accumulate_frame_history(C.byref(history.history), C.byref(device.app), C.byref(settings), C.byref(uploads.images(sequence[index], arena))) == 0
            assert_frame(history, arena, expected[index], True, (name, index))
    finally:
        history.close()
        uploads.free()
        arena.free()


def test_python_interface_takes_arrays_and_pointers(device):
    name = "saturating"
    width, height, _ = cases.SEQUENCES[name]
    sequence, expected = cases.build(name), cases.expected(name)
    history = device.create_frame_history(width, height)
    targets = [DeviceBuffer(width * height * 16) for _ in range(2)]
    position = DeviceBuffer(width * height * 16)
    try:
        position.upload(sequence[0]["position"])
        for index in range(3):
            frame = sequence[index]
            features = {"position": position.ptr if index == 1 else frame["position"], "normal": frame["normal"], "diffuse_albedo": frame["modulation"]}
            if index < 2:
                got = device.accumulate_history(frame["colour"], features, cases.settings(name), frame_history=history, want_variance=index == 0)
                assert got[0].tobytes() == expected[index][1].tobytes()
                assert (got[1] is None) if index else (got[1].tobytes() == expected[index][2].tobytes())
            else:
                assert history.accumulate(frame["colour"], features, cases.settings(name), out_colour=targets[0].ptr.value, out_variance=targets[1].ptr) is None
                device.sync()
                assert targets[0].download((height, width, 4), np.float32).tobytes() == expected[index][1].tobytes()
                assert targets[1].download((height, width, 4), np.float32).tobytes() == expected[index][2].tobytes()
            assert history.frame_count == index + 1
            images = history.read()
            assert all(images[key].tobytes() == expected[index][0][key].tobytes() for key in frame_history.HISTORY_IMAGES)
        with pytest.raises(ValueError):
            device.accumulate_history(sequence[0]["colour"][:8], features, frame_history=history)
        assert history.frame_count == 3
    finally:
        history.close()
        position.free()
        for target in targets:
            target.free()


# ---- 2. behind the pass ----------------------------------------------------------------------------------------------------

EXTENT = (83, 45)
TURN = math.radians(1.5)
HISTORY_SETTINGS = dict(max_length=32.0, sigma_depth=0.02, normal_threshold=0.9, spatial_length=4)
FILTER_SETTINGS = dict(iteration_count=3, normal_squarings=7, sigma_luminance=4.0, sigma_depth=0.02, variance_scale=1.0)
FEATURES = ("position", "normal", "diffuse_albedo", "reprojection")


def test_rendered_frames_are_accumulated_and_filtered_as_numpy_does(dataset):
    """Two cameras a small turn apart: each frame is rendered into a target of its own, its features and its reprojection
    under the previous camera's matrix by render_feature_buffers(), accumulate_frame_history(), and behind the second frame
    filter_frame() with variance_scale 1 - all queued without a wait in between; then the inputs are read back and numpy
    goes the same way: the same bits"""
    width, height = EXTENT
    shape, image_bytes = (height, width, 4), width * height * 16
    r = open_renderer(dataset, frames_in_flight=3)
    names = ("colour",) + FEATURES + ("accumulated", "variance")
    buffers = [{name: DeviceBuffer(image_bytes) for name in names} for _ in range(2)]
    filtered = {name: DeviceBuffer(image_bytes) for name in ("colour", "variance")}
    try:
        history = r.create_frame_history()
        assert (history.width, history.height) == EXTENT
        previous = feature_buffers.world_to_projection_space(r.constants())
        for index, images in enumerate(buffers):
            if index:
                r.app.scene_specification.camera.rotation_z += TURN
                r.render_visibility()
            r.render(images["colour"].ptr.value)
            features = {name: images[name].ptr.value for name in FEATURES}
            r.render_features(list(features), previous, pointers=features)
            assert history.accumulate(images["colour"].ptr.value, features, HISTORY_SETTINGS, out_colour=images["accumulated"].ptr.value,
                                      out_variance=images["variance"].ptr.value) is None
        r.filter_frame(buffers[1]["accumulated"].ptr.value, buffers[1]["variance"].ptr.value, features, FILTER_SETTINGS,
                       out_colour=filtered["colour"].ptr.value, out_variance=filtered["variance"].ptr.value)
        r.sync()
        host = [{name: images[name].download(shape, np.float32) for name in names} for images in buffers]
        state = frame_history.new_state(width, height)
        for index, images in enumerate(host):
            diagnostics = {}
            state, want_colour, want_variance = frame_history.accumulate(state, images["colour"], images["position"], images["normal"], images["reprojection"],
                                                                         images["diffuse_albedo"], HISTORY_SETTINGS, diagnostics)
            assert_same_bits(images["accumulated"], want_colour, ("accumulated", index))
            assert_same_bits(images["variance"], want_variance, ("variance", index))
        got = history.read()
        for key in frame_history.HISTORY_IMAGES:
            assert_same_bits(got[key], state[key], (key,))
        # the turn means something: most covered pixels find their history between pixels, some find none
        covered = host[1]["position"][..., 3] > 0
        print(diagnostics)
        assert 0.05 < covered.mean() < 0.95 and 0 < diagnostics["no_history"] < 0.5 * diagnostics["covered"]
        reprojection = host[1]["reprojection"]
        assert (reprojection[covered][:, 0] != np.floor(reprojection[covered][:, 0])).any() and (state["colour"][..., 3] == 2).any()
        assert np.isfinite(host[1]["colour"]).all() and want_variance[covered][:, :3].max() > 0
        want = frame_filter.filter_frame(want_colour, want_variance, host[1]["position"], host[1]["normal"], host[1]["diffuse_albedo"], FILTER_SETTINGS)
        assert_same_bits(filtered["colour"].download(shape, np.float32), want[0], ("filtered colour",))
        assert_same_bits(filtered["variance"].download(shape, np.float32), want[1], ("filtered variance",))
    finally:
        r.close()
        for buffer in [b for images in buffers for b in images.values()] + list(filtered.values()):
            buffer.free()


def test_radiance_target_between_frames_in_flight(dataset):
    """The radiance target itself as colour, queued between frames in flight: the call reads frame 2 - not frame 1, not
    frame 3, which waits for it - and the frames are those of a run without the call"""
    width, height = EXTENT
    shape, image_bytes = (height, width, 4), width * height * 16

    def run(with_history):
        r = open_renderer(dataset, frames_in_flight=3)
        names = ("position", "normal", "diffuse_albedo", "out_colour", "out_variance")
        buffers = {name: DeviceBuffer(image_bytes) for name in names}
        radiance, host = [], None
        try:
            features = {name: buffers[name].ptr.value for name in names[:3]}
            # (in both runs: with animated noise every upload of the constants, this call's too, takes the next seed)
            r.render_features(list(features), pointers=features)
            r.render()
            r.render()
            if with_history:
                assert r.accumulate_history(r.app.render_targets.radiance, features, HISTORY_SETTINGS, out_colour=buffers["out_colour"].ptr.value,
                                            out_variance=buffers["out_variance"].ptr.value) is None
            else:
                radiance.append(r.read_radiance())
            r.render()
            radiance.append(r.read_radiance())
            r.render()
            radiance.append(r.read_radiance())
            if with_history:
                r.sync()
                host = {name: buffers[name].download(shape, np.float32) for name in names}
        finally:
            r.close()
            for buffer in buffers.values():
                buffer.free()
        return radiance, host

    with_history, host = run(True)
    without = run(False)[0]
    second, third, fourth = without
    assert second.tobytes() != third.tobytes() and np.isfinite(second).all() and second[..., :3].max() > 0
    assert with_history[0].tobytes() == third.tobytes() and with_history[1].tobytes() == fourth.tobytes()
    fresh = frame_history.new_state(width, height)
    want = frame_history.accumulate(fresh, second, host["position"], host["normal"], None, host["diffuse_albedo"], HISTORY_SETTINGS)
    assert_same_bits(host["out_colour"], want[1], ("out_colour",))
    assert_same_bits(host["out_variance"], want[2], ("out_variance",))
    assert differing(want[1], frame_history.accumulate(fresh, third, host["position"], host["normal"], None, host["diffuse_albedo"], HISTORY_SETTINGS)[1]).any()


def test_arithmetic_mode_of_the_pass_changes_nothing(dataset):
    """The history is one build in one arithmetic: under a pass of any mode the same inputs give the same bytes, numpy's; the
    history has another extent (33x35) than the swapchain (16x16)"""
    name = "33x35"
    width, height, _ = cases.SEQUENCES[name]
    sequence, expected = cases.build(name), cases.expected(name)
    for arithmetic in ("libm", "exact", "fast"):
        r = open_renderer(dataset, arithmetic, extent=(16, 16))
        try:
            r.render()
            history = r.create_frame_history(width, height)
            assert (history.width, history.height) == (width, height) != (16, 16)
            for index in range(3):
                frame = sequence[index]
                features = {"position": frame["position"], "normal": frame["normal"], "reprojection": frame["reprojection"], "diffuse_albedo": frame["modulation"]}
                got_colour, got_variance = r.accumulate_history(frame["colour"], features, cases.settings(name), frame_history=history)
                assert got_colour.tobytes() == expected[index][1].tobytes() and got_variance.tobytes() == expected[index][2].tobytes(), (arithmetic, index)
        finally:
            r.close()


# ---- 3. the object and the refusals ------------------------------------------------------------------------------------------

def test_create_and_destroy_twice(device):
    lib = capi.load()
    e = device.app.swapchain.extent
    kept = (e.width, e.height)
    name = "33x35"
    try:
        e.width, e.height = 33, 35
        frame, want = cases.build(name)[0], cases.expected(name)[0]
        features = {"position": frame["position"], "normal": frame["normal"], "reprojection": frame["reprojection"], "diffuse_albedo": frame["modulation"]}
        for _ in range(2):
            # (0, 0: the swapchain extent)
            history = device.create_frame_history()
            assert (history.width, history.height) == (33, 35) and history.history.accumulated and history.frame_count == 0
            assert all(getattr(history.history, key)[i] for key in frame_history.HISTORY_IMAGES for i in range(2))
            assert not any(image.any() for image in history.read().values())
            assert device.accumulate_history(frame["colour"], features, cases.settings(name), frame_history=history)[0].tobytes() == want[1].tobytes()
            history.close()
            assert not history.history.accumulated and not history.history.colour[0] and history.history.width == 0
            # destroying what is destroyed does nothing
            lib.destroy_frame_history(C.byref(history.history), C.byref(device.app))
    finally:
        e.width, e.height = kept


def test_refusals_write_nothing(device, capfd):
    name = "saturating"
    width, height, _ = cases.SEQUENCES[name]
    sequence, expected = cases.build(name), cases.expected(name)
    arena, uploads = Arena(width, height), Uploads()
    history = device.create_frame_history(width, height)
    lib = capi.load()
    good = cases.settings(name)
    nan = float("nan")
    frame = dict(sequence[1], reprojection=cases.shift_image(width, height, 0, 0))
    try:
        assert lib.accumulate_frame_history(C.byref(history.history), C.byref(device.app), C.byref(settings_struct(good)), C.byref(uploads.images(sequence[0], arena))) == 0
        device.sync()
        arena.reset()
        before = history.read()

        def refused(settings=None, change=None, history_struct=None):
            images = uploads.images(frame, arena)
            if change:
                change(images)
            flush_c_output()
            capfd.readouterr()
            result = lib.accumulate_frame_history(C.byref(history_struct if history_struct is not None else history.history), C.byref(device.app),
                                                  C.byref(settings_struct(dict(good, **(settings or {})))), C.byref(images))
            flush_c_output()
            printed = capfd.readouterr().out
            assert result == 1 and printed.count("\n") == 1 and printed.endswith("\n"), (settings, printed)
            device.sync()
            assert arena.untouched(), (settings, printed)
            after = history.read()
            assert history.frame_count == 1 and all(before[key].tobytes() == after[key].tobytes() for key in before), (settings, printed)

        def set_member(member, value):
            return lambda images: setattr(images, member, value)
        for settings in [dict(max_length=0.5), dict(max_length=nan), dict(max_length=float("inf")), dict(sigma_depth=0.0), dict(sigma_depth=nan),
                         dict(sigma_depth=float("inf")), dict(normal_threshold=1.5), dict(normal_threshold=-1.5), dict(normal_threshold=nan), dict(spatial_length=65)]:
            refused(settings)
        for member in ("colour", "position", "normal", "out_colour"):
            refused(change=set_member(member, None))
        for member, _ in capi.FrameHistoryImages._fields_:
            refused(change=lambda images, member=member: setattr(images, member, getattr(images, member) + 4))
        # an output that overlaps an input - the same image, or its last pixel -, the other output or an image of the history
        for member in ("colour", "position", "normal", "reprojection", "modulation"):
            refused(change=lambda images, member=member: setattr(images, "out_colour", getattr(images, member)))
            refused(change=lambda images, member=member: setattr(images, "out_variance", getattr(images, member) + arena.image_bytes - 16))
        refused(change=lambda images: setattr(images, "out_variance", images.out_colour))
        refused(change=lambda images: setattr(images, "out_variance", images.out_colour - arena.image_bytes + 16))
        for key in frame_history.HISTORY_IMAGES:
            for i in range(2):
                refused(change=lambda images, key=key, i=i: setattr(images, "out_colour", getattr(history.history, key)[i]))
                refused(change=lambda images, key=key, i=i: setattr(images, "out_variance", getattr(history.history, key)[i] + arena.image_bytes - 16))
        # a history that was not created, or no longer is
        refused(history_struct=capi.FrameHistory())
        gone = device.create_frame_history(width, height)
        gone.close()
        refused(history_struct=gone.history)
        # (the same request is accepted once nothing is wrong with it)
        assert lib.accumulate_frame_history(C.byref(history.history), C.byref(device.app), C.byref(settings_struct(good)), C.byref(uploads.images(frame, arena))) == 0
        assert_frame(history, arena, expected[1], True, (name, 1))
    finally:
        history.close()
        uploads.free()
        arena.free()


# ---- 4. the command line -----------------------------------------------------------------------------------------------------

def test_command_line_writes_its_three_files(dataset, tmp_path, capfd):
    """python -m vulkan_renderer_amd.frame_history, called in this process, at 83x45: the last noisy frame, the accumulated
    and the filtered image, as Radiance files and as PNG files; accumulating changes the image, filtering changes it again"""
    width, height = EXTENT
    root = os.path.dirname(dataset["scene"])
    arguments = [root, "--width", str(width), "--height", str(height), "--spp", "1", "--frames", "4", "--turn", "3", "--max-length", "16"]
    assert frame_history.main(arguments + ["--filter", "--out", str(tmp_path / "hdr"), "--hdr"]) == 0
    assert frame_history.main(arguments + ["--filter", "--out", str(tmp_path / "png"), "--png"]) == 0
    assert frame_history.main(arguments + ["--out", str(tmp_path / "plain")]) == 0
    for directory, suffix in (("hdr", ".hdr"), ("png", ".png"), ("plain", ".hdr")):
        assert sorted(os.listdir(tmp_path / directory)) == sorted(name + suffix for name in ("noisy", "accumulated", "filtered"))
    files = {(directory, name): open(tmp_path / directory / (name + suffix), "rb").read()
             for directory, suffix in (("hdr", ".hdr"), ("png", ".png"), ("plain", ".hdr")) for name in ("noisy", "accumulated", "filtered")}
    for directory in ("hdr", "png"):
        assert len({files[(directory, name)] for name in ("noisy", "accumulated", "filtered")}) == 3
    # without --filter the third file is the accumulated image; the frames are the same in every run
    assert files[("plain", "filtered")] == files[("plain", "accumulated")] == files[("hdr", "accumulated")] and files[("plain", "noisy")] == files[("hdr", "noisy")]
    assert files[("hdr", "noisy")].startswith(b"#?RADIANCE")
    for name in ("noisy", "accumulated", "filtered"):
        assert np.asarray(png_cases.decode(files[("png", name)])).size == width * height * 3
    assert capfd.readouterr().out.count(" bytes)") == 9
