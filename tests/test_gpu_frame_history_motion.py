"""accumulate_moving_frame_history() (include/vkr_frame_history.h, "Moving geometry") on the device: the translating valleys
and every sequence of tests/frame_history_cases.py with pushed previous positions (tests/frame_history_motion_cases.py) frame
by frame against the numpy restatement in every bit, NULL previous_position against accumulate_frame_history(), the whole
chain behind a mesh that update_geometry() moves - motion buffers, history - against numpy's chain on the inputs read back,
and the refusals."""
import ctypes as C

import numpy as np
import pytest

import feature_buffer_cases as frames
import frame_history_motion_cases as cases
from helpers import Arena, DeviceBuffer, assert_same_bits, flush_c_output, open_renderer
from test_gpu_frame_history import Uploads, assert_frame, settings_struct
from vulkan_renderer_amd import capi, feature_buffers, frame_history, renderer, scene_update

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    """A renderer with nothing but its device: the history needs no scene and no pass"""
    r = renderer.Renderer()
    yield r
    r.close()


class MovingUploads(Uploads):
    """The images of a sequence on the device and, beside them, its previous_position images"""

    def previous(self, frame):
        image = frame["previous_position"]
        if id(image) not in self.buffers:
            self.buffers[id(image)] = (DeviceBuffer(max(image.nbytes, 16)), image)
            self.buffers[id(image)][0].upload(image)
        return self.buffers[id(image)][0].ptr.value


# ---- 1. the sequences against numpy --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cases.NAMES)
def test_sequences_equal_numpy_in_every_bit(device, name):
    """Frame by frame, two histories side by side: one with out_variance (and the second launch, unless the spatial length
    is 0), one without, whose variance image must stay untouched"""
    if name in cases.VALLEYS:
        cases.assert_valley_conditions(name)
    width, height = cases.extent(name)
    sequence, expected = cases.frames_of(name), cases.expected(name)
    # (the previous positions mean something: numpy's own results differ from those without them)
    assert any(a[0]["colour"].tobytes() != b[0]["colour"].tobytes() for a, b in zip(expected, cases.expected(name, moving=False)))
    arena, uploads = Arena(width, height), MovingUploads()
    histories = {True: device.create_frame_history(width, height), False: device.create_frame_history(width, height)}
    lib = capi.load()
    try:
        settings = settings_struct(cases.settings(name))
        for index, frame in enumerate(sequence):
            for want_variance, history in histories.items():
                arena.reset()
                images = uploads.images(frame, arena, want_variance)
                assert lib.accumulate_moving_frame_history(C.byref(history.history), C.byref(device.app), C.byref(settings), C.byref(images), uploads.previous(frame)) == 0
                assert_frame(history, arena, expected[index], want_variance, (name, index, want_variance))
    finally:
        for history in histories.values():
            history.close()
        uploads.free()
        arena.free()


@pytest.mark.parametrize("name", ["valley_83x45", "fraction", "7x3"])
def test_null_previous_position_gives_the_bytes_of_accumulate_frame_history(device, name):
    """On the same inputs, one history through each entry point: the outputs and the four history images, byte for byte -
    which are numpy's without previous_position"""
    width, height = cases.extent(name)
    sequence, expected = cases.frames_of(name), cases.expected(name, moving=False)
    arenas, uploads = [Arena(width, height), Arena(width, height)], MovingUploads()
    histories = [device.create_frame_history(width, height), device.create_frame_history(width, height)]
    lib = capi.load()
    try:
        settings = settings_struct(cases.settings(name))
        for index, frame in enumerate(sequence):
            for arena in arenas:
                arena.reset()
            assert lib.accumulate_frame_history(C.byref(histories[0].history), C.byref(device.app), C.byref(settings), C.byref(uploads.images(frame, arenas[0]))) == 0
            assert lib.accumulate_moving_frame_history(C.byref(histories[1].history), C.byref(device.app), C.byref(settings), C.byref(uploads.images(frame, arenas[1])), None) == 0
            a, b = arenas[0].read(), arenas[1].read()
            assert a[2] and b[2] and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (name, index)
            read = [history.read() for history in histories]
            assert all(read[0][key].tobytes() == read[1][key].tobytes() for key in frame_history.HISTORY_IMAGES), (name, index)
            assert_frame(histories[1], arenas[1], expected[index], True, (name, index))
    finally:
        for history in histories:
            history.close()
        uploads.free()
        for arena in arenas:
            arena.free()


def test_python_interface_takes_previous_position(device):
    name = "valley_16x16"
    width, height = cases.extent(name)
    sequence, expected = cases.frames_of(name), cases.expected(name)
    history = device.create_frame_history(width, height)
    previous = DeviceBuffer(width * height * 16)
    try:
        for index in range(3):
            frame = sequence[index]
            previous.upload(frame["previous_position"])
            features = {"position": frame["position"], "normal": frame["normal"], "reprojection": frame["reprojection"],
                        "previous_position": previous.ptr.value if index == 1 else frame["previous_position"]}
            colour, variance = device.accumulate_history(frame["colour"], features, cases.settings(name), frame_history=history)
            assert colour.tobytes() == expected[index][1].tobytes() and variance.tobytes() == expected[index][2].tobytes(), index
        assert (history.read()["colour"][..., 3].max(), history.frame_count) == (3.0, 3)
    finally:
        history.close()
        previous.free()


# ---- 2. behind a mesh that moves -------------------------------------------------------------------------------------------

EXTENT = (83, 45)
END_TO_END_FRAMES = 4
# per frame, in codes: 15 cm up - the box of the mesh is a little more than 1 m high -, a few millimetres sideways
RISE = np.array([1000, -700, 270000], np.int64)
HISTORY_SETTINGS = dict(max_length=32.0, sigma_depth=0.02, normal_threshold=0.9, spatial_length=4)
FEATURES = ("position", "normal", "diffuse_albedo", "reprojection")


def mean_length(state, where):
    return float(state["colour"][..., 3][where].astype(np.float64).mean())


def test_history_follows_update_geometry_as_numpy_does(dataset):
    """Four frames under a camera 60 cm above the ground while the whole mesh rises by RISE per frame: render, keep the old
    positions, update_geometry (refit), visibility pass, render, render_features and render_motion, then one history with the
    motion buffers and one with the camera-only reprojection of render_features - all queued; then the inputs are read back
    and numpy goes the same way.  Numpy's chain is asserted to mean something first: the history with motion buffers is
    longer than the other and at least 2 by the last frame, over the covered pixels whose previous position is in the frame."""
    width, height = EXTENT
    shape, image_bytes = (height, width, 4), width * height * 16
    r = open_renderer(dataset, frames_in_flight=3)
    names = ("colour",) + FEATURES + ("motion_reprojection", "previous_position", "with_motion", "with_motion_variance", "camera_only", "camera_only_variance")
    buffers = [{name: DeviceBuffer(image_bytes) for name in names} for _ in range(END_TO_END_FRAMES)]
    try:
        frames.set_camera(r, frames.SECOND_CAMERA)
        histories = {"with_motion": r.create_frame_history(), "camera_only": r.create_frame_history()}
        words = r.host_inputs()["quantized_positions"]
        codes = scene_update.unpack_positions(words).astype(np.int64)
        matrix = feature_buffers.world_to_projection_space(r.constants())
        previous_words, all_words = None, []
        for index, images in enumerate(buffers):
            if index:
                r.finish_frames()
                previous_words = words
                words = scene_update.pack_positions(np.clip(codes + index * RISE, 0, scene_update.CODE_MAX).astype(np.uint32))
                assert not r.update_geometry(words, policy="refit")["rebuilt"]
            r.render_visibility()
            r.render(images["colour"].ptr.value)
            features = {name: images[name].ptr.value for name in FEATURES}
            r.render_features(list(features), matrix, pointers=features)
            assert r.render_motion(previous_words, matrix, ["reprojection", "previous_position"],
                                   pointers={"reprojection": images["motion_reprojection"].ptr.value, "previous_position": images["previous_position"].ptr.value}) is None
            moving = dict(features, reprojection=images["motion_reprojection"].ptr.value, previous_position=images["previous_position"].ptr.value)
            assert histories["with_motion"].accumulate(images["colour"].ptr.value, moving, HISTORY_SETTINGS, out_colour=images["with_motion"].ptr.value,
                                                       out_variance=images["with_motion_variance"].ptr.value) is None
            assert histories["camera_only"].accumulate(images["colour"].ptr.value, features, HISTORY_SETTINGS, out_colour=images["camera_only"].ptr.value,
                                                       out_variance=images["camera_only_variance"].ptr.value) is None
            all_words.append(words)
        r.sync()
        host = [{name: images[name].download(shape, np.float32) for name in names} for images in buffers]
        got = {key: history.read() for key, history in histories.items()}
    finally:
        r.close()
        for buffer in [b for images in buffers for b in images.values()]:
            buffer.free()
    # numpy's chain on the inputs read back, and what it has to show
    states = {key: frame_history.new_state(width, height) for key in histories}
    results, lengths = [], []
    for index, images in enumerate(host):
        arguments = (images["colour"], images["position"], images["normal"])
        with_motion = frame_history.accumulate(states["with_motion"], *arguments, images["motion_reprojection"], images["diffuse_albedo"], HISTORY_SETTINGS, None, images["previous_position"])
        camera_only = frame_history.accumulate(states["camera_only"], *arguments, images["reprojection"], images["diffuse_albedo"], HISTORY_SETTINGS)
        states = {"with_motion": with_motion[0], "camera_only": camera_only[0]}
        results.append({"with_motion": with_motion, "camera_only": camera_only})
        found = (images["position"][..., 3] > 0) & (images["motion_reprojection"][..., 3] == 1)
        lengths.append((mean_length(with_motion[0], found), mean_length(camera_only[0], found), int(found.sum())))
    print("mean history length with motion buffers, camera only, pixels:", lengths)
    assert len({w.tobytes() for w in all_words}) == END_TO_END_FRAMES and lengths[0][:2] == (1.0, 1.0)
    for with_motion, camera_only, pixels in lengths[1:]:
        assert pixels > 500 and with_motion > camera_only
    assert lengths[-1][0] >= 2.0
    # the device against it, in every bit
    for index, images in enumerate(host):
        for key in ("with_motion", "camera_only"):
            assert_same_bits(images[key], results[index][key][1], (key, index))
            assert_same_bits(images[key + "_variance"], results[index][key][2], (key, "variance", index))
    for key in ("with_motion", "camera_only"):
        for image in frame_history.HISTORY_IMAGES:
            assert_same_bits(got[key][image], states[key][image], (key, image))


def test_command_line_moves_the_mesh(dataset, tmp_path, capfd):
    """python -m vulkan_renderer_amd.frame_history --move, called in this process, at 83x45: three files per run, the
    accumulated image with the motion buffers is another than with --no-motion, and a mesh that moves gives other frames than
    one that rests"""
    import os
    root = os.path.dirname(dataset["scene"])
    arguments = [root, "--width", "83", "--height", "45", "--spp", "1", "--frames", "4", "--max-length", "16", "--filter"]
    assert frame_history.main(arguments + ["--move", "0.05", "--out", str(tmp_path / "motion")]) == 0
    assert frame_history.main(arguments + ["--move", "0.05", "--no-motion", "--out", str(tmp_path / "camera")]) == 0
    assert frame_history.main(arguments + ["--out", str(tmp_path / "rest")]) == 0
    files = {(directory, name): open(tmp_path / directory / (name + ".hdr"), "rb").read()
             for directory in ("motion", "camera", "rest") for name in ("noisy", "accumulated", "filtered")}
    assert all(data.startswith(b"#?RADIANCE") for data in files.values())
    assert files[("motion", "noisy")] != files[("rest", "noisy")] and files[("motion", "accumulated")] != files[("camera", "accumulated")]
    assert len({files[("motion", name)] for name in ("noisy", "accumulated", "filtered")}) == 3
    assert capfd.readouterr().out.count(" bytes)") == 9


# ---- 3. the refusals -----------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_history_intact(device, capfd):
    name = "valley_16x16"
    width, height = cases.extent(name)
    sequence, expected = cases.frames_of(name), cases.expected(name)
    arena, uploads = Arena(width, height), MovingUploads()
    history = device.create_frame_history(width, height)
    lib = capi.load()
    settings = settings_struct(cases.settings(name))
    try:
        assert lib.accumulate_moving_frame_history(C.byref(history.history), C.byref(device.app), C.byref(settings), C.byref(uploads.images(sequence[0], arena)), uploads.previous(sequence[0])) == 0
        device.sync()
        arena.reset()
        before = history.read()
        frame = sequence[1]

        def refused(previous=None, change=None):
            images = uploads.images(frame, arena)
            if change:
                change(images)
            flush_c_output()
            capfd.readouterr()
            result = lib.accumulate_moving_frame_history(C.byref(history.history), C.byref(device.app), C.byref(settings), C.byref(images),
                                                         uploads.previous(frame) if previous is None else previous)
            flush_c_output()
            printed = capfd.readouterr().out
            assert result == 1 and printed.count("\n") == 1 and printed.startswith("accumulate_moving_frame_history()"), printed
            device.sync()
            assert arena.untouched(), printed
            after = history.read()
            assert history.frame_count == 1 and all(before[key].tobytes() == after[key].tobytes() for key in before), printed

        # misaligned; an output on it, or on its last pixel
        refused(previous=uploads.previous(frame) + 8)
        refused(previous=arena.address(0))
        refused(previous=arena.address(1) + arena.image_bytes - 16)
        refused(change=lambda images: setattr(images, "out_colour", uploads.previous(frame)))
        refused(change=lambda images: setattr(images, "out_variance", uploads.previous(frame) + arena.image_bytes - 16))
        # what accumulate_frame_history() refuses, under this name
        refused(change=lambda images: setattr(images, "colour", None))
        refused(change=lambda images: setattr(images, "out_variance", images.out_colour))
        # (the same request is accepted once nothing is wrong with it)
        assert lib.accumulate_moving_frame_history(C.byref(history.history), C.byref(device.app), C.byref(settings), C.byref(uploads.images(frame, arena)), uploads.previous(frame)) == 0
        assert_frame(history, arena, expected[1], True, (name, 1))
    finally:
        history.close()
        uploads.free()
        arena.free()
