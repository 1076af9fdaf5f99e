"""Motion buffers (include/vkr_motion_buffers.h) on the device: the three images of every mesh of
tests/motion_buffer_cases.py in every frame against the numpy restatement (vulkan_renderer_amd/motion_buffers.py), bit for
bit in the libm and the polynomial mode and between guard bytes; subsets; the feature buffers' reprojection where nothing
moved, in every arithmetic mode; host arrays and device addresses; independence of the frames of the pass; the fast mode
against libm; the refusals; the Python interface and the command line.  The conditions that the meshes are chosen for are
asserted on the numpy side (tests/motion_buffer_cases.py, and without a GPU in tests/test_motion_buffers.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import feature_buffer_cases as frames
import motion_buffer_cases as cases
from helpers import GUARD_BYTE, GUARD_BYTES, DeviceBuffer, assert_same_bits, flush_c_output
from vulkan_renderer_amd import capi, feature_buffers, motion_buffers, renderer

pytestmark = pytest.mark.gpu

NAMES = capi.MOTION_IMAGES
FRAMES = {"83x45": (83, 45), "16x16": (16, 16), "7x3": (7, 3)}

# Fast mode against libm on the device: the largest absolute difference per image over the three frames and the four meshes
# (channels x, y, z, w together), measured on an MI355X (profiles/r33_summary.md).  As in tests/test_gpu_feature_buffers.py
# the frames are few and what the fast mode costs depends on the geometry, so the test allows four times as much.
FAST_MEASURED = {
    "reprojection": 2.738,            # (83x45, still: X of a point next to the second camera's plane c_3 = 0, the figure of the
                                      # feature buffers; rigid 0.34, per_triangle 0.48, large 1.5e-4; 16x16 2.8e-5, 7x3 1.9e-6)
    "previous_position": 1.287e-5,    # (16x16, per_triangle; 83x45 1.4e-6, 7x3 9.5e-7)
    "motion": 2.738,                  # (per frame and mesh the figure of the reprojection: its X - x and Y - y)
}


def open_renderer(dataset, key, arithmetic="libm", **arguments):
    """A renderer with targets, pass and visibility of frame `key`"""
    r = renderer.Renderer(arithmetic=arithmetic, **arguments)
    width, height = FRAMES[key]
    frames.apply_frame(r, dataset, width, height)
    r.create_targets()
    r.create_pass()
    r.render_visibility()
    return r


class ImageArena:
    """[guard][reprojection][guard][previous_position][guard][motion][guard] in one allocation"""

    def __init__(self, width, height):
        self.shape, self.image_bytes = (height, width, 4), width * height * 16
        self.stride = GUARD_BYTES + self.image_bytes
        self.buffer = DeviceBuffer(len(NAMES) * self.stride + GUARD_BYTES)
        self.reset()

    def reset(self):
        self.buffer.upload(np.full(self.buffer.nbytes, GUARD_BYTE, np.uint8))

    def address(self, name):
        return self.buffer.ptr.value + GUARD_BYTES + NAMES.index(name) * self.stride

    def read(self, written):
        """-> {name: image} of the names in `written`; asserts that every other byte is a guard byte"""
        after = self.buffer.download((self.buffer.nbytes,), np.uint8)
        images, untouched = {}, np.ones(after.shape, bool)
        for name in written:
            first = GUARD_BYTES + NAMES.index(name) * self.stride
            images[name] = after[first:first + self.image_bytes].view(np.float32).reshape(self.shape)
            untouched[first:first + self.image_bytes] = False
        assert (after[untouched] == GUARD_BYTE).all(), written
        return images

    def free(self):
        self.buffer.free()


_rendered = {}


def rendered(dataset, key, arithmetic):
    """-> {mesh: (images of the device, expected images or None in the fast mode)}, "visibility" and "null": the images with
    previous_positions NULL under the second camera; rendered once per module, left unchanged"""
    if (key, arithmetic) not in _rendered:
        width, height = FRAMES[key]
        r, arena = open_renderer(dataset, key, arithmetic), ImageArena(width, height)
        try:
            visibility = r.read_visibility()
            result = {"visibility": visibility}
            pointers = {name: arena.address(name) for name in NAMES}
            for name in cases.MESHES:
                expected, counts, previous, matrix = cases.expected(r, visibility, name)
                arena.reset()
                assert r.render_motion(previous, matrix, pointers=pointers) is None
                r.sync()
                result[name] = (arena.read(NAMES), expected, counts)
            result["null"] = r.render_motion(None, frames.second_matrix(r))
        finally:
            r.close()
            arena.free()
        _rendered[(key, arithmetic)] = result
    return _rendered[(key, arithmetic)]


# ---- 1. the IEEE modes against numpy -----------------------------------------------------------------------------------

def test_meshes_meet_their_conditions(dataset):
    """(on the visibility of the device: what the comparisons below mean something for)"""
    results = {}
    for key, extent in FRAMES.items():
        frame = rendered(dataset, key, "libm")
        for name in cases.MESHES:
            results[(name, extent)] = (frame[name][1], frame[name][2], frame["visibility"])
    cases.assert_conditions(results)


@pytest.mark.parametrize("key", list(FRAMES))
@pytest.mark.parametrize("arithmetic", ["libm", "exact"])
def test_images_equal_numpy_in_every_bit(dataset, key, arithmetic):
    frame = rendered(dataset, key, arithmetic)
    for name in cases.MESHES:
        got, expected, _ = frame[name]
        for image in NAMES:
            assert got[image].shape == expected[image].shape
            assert_same_bits(got[image], expected[image], (key, arithmetic, name, image))
    # the device itself sees no motion where there is none
    assert motion_buffers.count_pixels(frame["still"][0])["moved"] == 0
    assert motion_buffers.count_pixels(frame["rigid"][0]) == frame["rigid"][2]


# ---- 2. subsets ------------------------------------------------------------------------------------------------------

def test_one_image_at_a_time_and_nothing_else_is_written(dataset):
    key = "83x45"
    together = rendered(dataset, key, "libm")["per_triangle"][0]
    r, arena = open_renderer(dataset, key), ImageArena(*FRAMES[key])
    try:
        _, _, previous, matrix = cases.expected(r, r.read_visibility(), "per_triangle")
        for name in NAMES:
            arena.reset()
            assert r.render_motion(previous, matrix, [name], pointers={name: arena.address(name)}) is None
            r.sync()
            assert arena.read([name])[name].tobytes() == together[name].tobytes(), name
    finally:
        r.close()
        arena.free()


# ---- 3. nothing moved: the reprojection of the feature buffers -------------------------------------------------------

@pytest.mark.parametrize("arithmetic", ["libm", "exact", "fast"])
def test_null_and_equal_positions_give_the_feature_buffers_reprojection(dataset, arithmetic):
    for key in FRAMES:
        r = open_renderer(dataset, key, arithmetic)
        try:
            second = frames.second_matrix(r)
            want = r.render_features(["reprojection"], second)["reprojection"]
            words = r.host_inputs()["quantized_positions"]
            for previous in (None, words, int(r.app.scene.mesh.positions)):
                got = r.render_motion(previous, second)
                assert got["reprojection"].tobytes() == want.tobytes(), (key, arithmetic, type(previous))
                assert motion_buffers.count_pixels(got)["moved"] == 0
            covered = r.read_visibility() != 0xFFFFFFFF
            assert covered.any() and (want[..., 3][covered] == 0).any() and (want[..., 3][covered] == 1).any()
        finally:
            r.close()
    if arithmetic != "fast":
        assert rendered(dataset, "83x45", arithmetic)["null"]["reprojection"].tobytes() == rendered(dataset, "83x45", arithmetic)["still"][0]["reprojection"].tobytes()


def test_host_array_and_device_address_give_the_same_bytes(dataset):
    key = "83x45"
    from_array = rendered(dataset, key, "libm")["per_triangle"][0]
    r = open_renderer(dataset, key)
    try:
        _, _, previous, matrix = cases.expected(r, r.read_visibility(), "per_triangle")
        on_device = DeviceBuffer(previous.nbytes)
        on_device.upload(previous)
        for address in (on_device.ptr.value, on_device.ptr):
            got = r.render_motion(address, matrix)
            for name in NAMES:
                assert got[name].tobytes() == from_array[name].tobytes(), name
        on_device.free()
    finally:
        r.close()


# ---- 4. independence of the pass --------------------------------------------------------------------------------------

def test_motion_calls_leave_the_frames_alone(dataset):
    """The check of test_feature_calls_leave_the_frames_alone: motion images before any frame, after one and between two
    frames in flight are the same images, and the frames are those of a run without the calls"""
    key = "83x45"
    width, height = FRAMES[key]

    def run(with_motion):
        r = open_renderer(dataset, key, frames_in_flight=3)
        images, radiance = [], []
        try:
            _, _, previous, matrix = cases.expected(r, r.read_visibility(), "per_triangle")

            def take():
                if with_motion:
                    images.append(r.render_motion(previous, matrix))
            take()  # before any frame
            r.render()
            radiance.append(r.read_radiance())
            take()  # after one
            r.render()
            if with_motion:
                # between two frames in flight: queued without waiting for them
                kept = {name: DeviceBuffer(width * height * 16) for name in NAMES}
                on_device = DeviceBuffer(previous.nbytes)
                on_device.upload(previous)
                r.render_motion(on_device.ptr.value, matrix, pointers={name: buffer.ptr.value for name, buffer in kept.items()})
            r.render()
            radiance.append(r.read_radiance())
            if with_motion:
                r.sync()
                images.append({name: buffer.download((height, width, 4), np.float32) for name, buffer in kept.items()})
                for buffer in list(kept.values()) + [on_device]:
                    buffer.free()
        finally:
            r.close()
        return images, radiance

    images, frames_with = run(True)
    _, frames_without = run(False)
    assert len(images) == 3
    want = rendered(dataset, key, "libm")["per_triangle"][0]
    for taken in images:
        for name in NAMES:
            assert taken[name].tobytes() == want[name].tobytes(), name
    for a, b in zip(frames_with, frames_without):
        assert a.tobytes() == b.tobytes() and np.isfinite(a).all() and a[..., :3].max() > 0


# ---- 5. the fast mode --------------------------------------------------------------------------------------------------

def test_fast_mode_stays_near_libm(dataset):
    largest = {name: 0.0 for name in FAST_MEASURED}
    for key in FRAMES:
        fast, libm = rendered(dataset, key, "fast"), rendered(dataset, key, "libm")
        covered = libm["visibility"] != 0xFFFFFFFF
        assert np.array_equal(fast["visibility"], libm["visibility"])
        for mesh in cases.MESHES:
            for name in FAST_MEASURED:
                a, b = fast[mesh][0][name], libm[mesh][0][name]
                assert np.isfinite(a[covered]).all(), (key, mesh, name)
                assert a[~covered].tobytes() == b[~covered].tobytes(), (key, mesh, name)
                difference = float(np.abs(a[covered].astype(np.float64) - b[covered].astype(np.float64)).max())
                print(key, mesh, name, "largest difference of the fast mode from libm: %.3e" % difference)
                largest[name] = max(largest[name], difference)
    print("over the frames and meshes:", {name: "%.3e" % value for name, value in largest.items()})
    for name, value in largest.items():
        assert value <= 4.0 * FAST_MEASURED[name], (name, value)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------

def test_refusals_print_one_line_and_write_nothing(dataset, capfd):
    key = "16x16"
    width, height = FRAMES[key]
    arena = ImageArena(width, height)
    lib = capi.load()

    def request(**members):
        buffers = capi.MotionBuffers()
        for i in range(4):
            buffers.previous_matrix[i][i] = 1.0
        for name, value in members.items():
            setattr(buffers, name, value)
        return buffers

    def refused(r, buffers):
        flush_c_output()
        capfd.readouterr()
        result = lib.render_motion_buffers(C.byref(r.app), C.byref(buffers))
        flush_c_output()
        printed = capfd.readouterr().out
        assert result == 1 and printed.count("\n") == 1 and printed.startswith("render_motion_buffers()"), printed
        r.sync()
        arena.read([])

    try:
        # no pass; a pass but no targets
        r = renderer.Renderer()
        frames.apply_frame(r, dataset, width, height)
        refused(r, request(reprojection=arena.address("reprojection")))
        r.create_pass()
        refused(r, request(reprojection=arena.address("reprojection")))
        r.close()
        r = open_renderer(dataset, key)
        try:
            positions = int(r.app.scene.mesh.positions)
            refused(r, request())
            refused(r, request(previous_positions=positions))
            for name in NAMES:
                refused(r, request(**{name: arena.address(name) + 8}))
            refused(r, request(reprojection=arena.address("reprojection"), motion=arena.address("motion") + 4))
            refused(r, request(previous_positions=positions + 4, reprojection=arena.address("reprojection")))
            r.set_tiles(tile_size=16, rank=0, rank_count=2)
            refused(r, request(reprojection=arena.address("reprojection")))
            r.set_tiles(tile_size=16, rank=0, rank_count=1, slab_layout=True)
            refused(r, request(reprojection=arena.address("reprojection")))
            r.set_tiles(tile_size=0, rank=0, rank_count=1, slab_layout=False)
            # (the same request is accepted once nothing is wrong with it)
            assert lib.render_motion_buffers(C.byref(r.app), C.byref(request(previous_positions=positions, reprojection=arena.address("reprojection")))) == 0
            r.sync()
            assert arena.read(["reprojection"])["reprojection"].tobytes() != bytes([GUARD_BYTE]) * arena.image_bytes
            with pytest.raises(ValueError):
                r.render_motion(None, np.eye(4), ["depth"])
            with pytest.raises(ValueError):
                r.render_motion(np.zeros((5, 2), np.uint32), np.eye(4))
        finally:
            r.close()
    finally:
        arena.free()


# ---- 7. the command line -----------------------------------------------------------------------------------------------

def test_command_line_writes_the_images_of_a_moved_mesh(dataset, tmp_path, capfd):
    """python -m vulkan_renderer_amd.motion_buffers, called in this process: the arrays of --npy are the images of
    render_motion() for the same motion, and numpy's for the inputs read back"""
    from vulkan_renderer_amd import scene_update
    root = os.path.dirname(dataset["scene"])
    assert motion_buffers.main([root, "--config", "3", "--width", "83", "--height", "45", "--amplitude", "0.05", "--npy", str(tmp_path)]) == 0
    printed = capfd.readouterr().out
    r = renderer.Renderer()
    try:
        renderer.setup_config(r, 3, dataset, 83, 45, acceleration_structure=True)
        r.create_targets()
        r.create_pass()
        matrix = feature_buffers.world_to_projection_space(r.constants())
        motion = scene_update.Wobble(r, 0.05)
        r.update_geometry(motion.words(0))
        r.render_visibility()
        images = r.render_motion(motion.rest_words, matrix)
        inputs, visibility = r.host_inputs(), r.read_visibility()
    finally:
        r.close()
    counts = {}
    want = motion_buffers.expected_images(visibility, inputs["quantized_positions"], motion.rest_words, inputs["constants"], matrix, counts)
    assert np.array_equal(inputs["quantized_positions"], motion.words(0))
    for name in NAMES:
        assert np.load(tmp_path / (name + ".npy")).tobytes() == images[name].tobytes() == want[name].tobytes(), name
    assert motion_buffers.count_pixels(images) == counts and 0 < counts["moved"] <= counts["covered"] and counts["inside"] > 0
    assert "%d pixels moved" % counts["moved"] in printed
