"""The frame filter (include/vkr_frame_filter.h) on the device: every case of tests/frame_filter_cases.py against the numpy
restatement in every bit of both outputs and between guard bytes, the filter behind a rendered, accumulated frame and on the
radiance target between frames in flight, the three arithmetic modes of the pass, the refusals and the command line."""
import ctypes as C
import os

import numpy as np
import pytest

import frame_filter_cases as cases
import png_cases
from helpers import GUARD_BYTE, Arena, DeviceBuffer, differing, flush_c_output, open_renderer
from vulkan_renderer_amd import capi, frame_filter, renderer

pytestmark = pytest.mark.gpu

INPUT_NAMES = ("colour", "variance", "position", "normal", "modulation")


@pytest.fixture(scope="module")
def device():
    """A renderer with nothing but its device: the filter needs no scene and no pass"""
    r = renderer.Renderer()
    yield r
    r.close()


class FilterArena(Arena):
    """The guarded outputs, and the inputs of a case in buffers of their own"""

    def __init__(self, width, height, images):
        super().__init__(width, height)
        self.inputs = {}
        for name in INPUT_NAMES:
            if images.get(name) is not None:
                self.inputs[name] = DeviceBuffer(self.image_bytes)
                self.inputs[name].upload(images[name])

    def images(self, want_variance=True):
        pointers = {name: (self.inputs[name].ptr.value if name in self.inputs else None) for name in INPUT_NAMES}
        return capi.FrameFilterImages(pointers["colour"], pointers["variance"], pointers["position"], pointers["normal"], pointers["modulation"],
                                      self.address(0), self.address(1) if want_variance and "variance" in self.inputs else None)

    def free(self):
        super().free()
        for buffer in self.inputs.values():
            buffer.free()


def settings_struct(values):
    return capi.FrameFilterSettings(int(values["iteration_count"]), int(values["normal_squarings"]), float(values["sigma_luminance"]),
                                    float(values["sigma_depth"]), float(values["variance_scale"]))


# ---- 1. the cases against numpy ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("iteration_count", cases.ITERATION_COUNTS)
@pytest.mark.parametrize("name", list(cases.CASES))
def test_cases_equal_numpy_in_every_bit(device, name, iteration_count):
    """Both outputs in every bit, between guard bytes; then the colour alone (no variance output): the same bytes, the
    variance's place untouched.  Both kernels run in every case of two or more iterations: the first launch from its LDS tile
    (alone with one iteration: it then finishes too), the later ones from global memory.  Neither has a threshold: frames
    smaller than a workgroup's tile (7x3, 5x9 with a modulation image), of exactly one (16x16) and of several with partial
    ones on both edges go the same way."""
    cases.assert_conditions(name)
    width, height = cases.CASES[name][:2]
    images = cases.inputs(name)
    want_colour, want_variance, _ = cases.expected(name, iteration_count)
    arena = FilterArena(width, height, images)
    filter_ = device.create_frame_filter(width, height)
    lib = capi.load()
    try:
        settings = settings_struct(cases.settings(name, iteration_count))
        assert lib.filter_frame(C.byref(filter_.filter), C.byref(device.app), C.byref(settings), C.byref(arena.images())) == 0
        device.sync()
        got_colour, got_variance, guards_intact = arena.read()
        assert guards_intact
        different = differing(got_colour, want_colour)
        print(name, iteration_count, "colour pixels that differ:", int(different.sum()))
        assert not different.any(), (np.argwhere(different)[:4].tolist(), got_colour[different][:2], want_colour[different][:2])
        if want_variance is not None:
            different = differing(got_variance, want_variance)
            print(name, iteration_count, "variance pixels that differ:", int(different.sum()))
            assert not different.any(), (np.argwhere(different)[:4].tolist(), got_variance[different][:2], want_variance[different][:2])
        else:
            assert (got_variance.view(np.uint8) == GUARD_BYTE).all()
        arena.reset()
        assert lib.filter_frame(C.byref(filter_.filter), C.byref(device.app), C.byref(settings), C.byref(arena.images(want_variance=False))) == 0
        device.sync()
        got_colour, got_variance, guards_intact = arena.read()
        assert guards_intact and got_colour.tobytes() == want_colour.tobytes() and (got_variance.view(np.uint8) == GUARD_BYTE).all()
    finally:
        filter_.close()
        arena.free()


def test_python_interface_takes_arrays_and_pointers(device):
    name = "16x16"
    images = cases.inputs(name)
    want_colour, want_variance, _ = cases.expected(name, 2)
    filter_ = device.create_frame_filter(16, 16)
    target = DeviceBuffer(16 * 16 * 16)
    try:
        features = {"position": images["position"], "normal": images["normal"], "diffuse_albedo": images["modulation"]}
        got = device.filter_frame(images["colour"], images["variance"], features, cases.settings(name, 2), frame_filter=filter_)
        assert got[0].tobytes() == want_colour.tobytes() and got[1].tobytes() == want_variance.tobytes()
        assert device.filter_frame(images["colour"], images["variance"], features, cases.settings(name, 2), out_colour=target.ptr.value, frame_filter=filter_) is None
        device.sync()
        assert target.download((16, 16, 4), np.float32).tobytes() == want_colour.tobytes()
        with pytest.raises(ValueError):
            device.filter_frame(images["colour"][:8], None, features, frame_filter=filter_)
    finally:
        filter_.close()
        target.free()


# ---- 2. behind the pass ----------------------------------------------------------------------------------------------------

EXTENT = (83, 45)
FRAME_SETTINGS = dict(iteration_count=5, normal_squarings=7, sigma_luminance=4.0, sigma_depth=0.02)


def test_rendered_frames_are_filtered_as_numpy_filters_them(dataset):
    """Four frames of render_shading_pass() in a ring of targets, accumulate_frames(), the mean and the variance of
    resolve_frame_statistics(), position, normal and albedo of render_feature_buffers(), filter_frame() - all queued without
    a wait in between; then the inputs are read back and numpy filters them: the same bits"""
    width, height = EXTENT
    shape, image_bytes, frame_count = (height, width, 4), width * height * 16, 4
    r = open_renderer(dataset, frames_in_flight=3)
    names = ("mean", "variance", "position", "normal", "diffuse_albedo", "out_colour", "out_variance")
    buffers = {name: DeviceBuffer(image_bytes) for name in names}
    ring = [DeviceBuffer(image_bytes) for _ in range(frame_count)]
    try:
        statistics = r.create_statistics(width * height)
        for target in ring:
            r.render(target.ptr.value)
        statistics.accumulate([target.ptr.value for target in ring])
        statistics.resolve(buffers["mean"].ptr.value, buffers["variance"].ptr.value)
        features = {name: buffers[name].ptr.value for name in ("position", "normal", "diffuse_albedo")}
        r.render_features(list(features), pointers=features)
        settings = dict(FRAME_SETTINGS, variance_scale=1.0 / frame_count)
        assert r.filter_frame(buffers["mean"].ptr.value, buffers["variance"].ptr.value, features, settings,
                              out_colour=buffers["out_colour"].ptr.value, out_variance=buffers["out_variance"].ptr.value) is None
        r.sync()
        host = {name: buffers[name].download(shape, np.float32) for name in names}
        covered = host["position"][..., 3] > 0
        assert 0.05 < covered.mean() < 0.95 and host["variance"][covered][:, :3].max() > 0 and np.isfinite(host["mean"]).all()
        want_colour, want_variance = frame_filter.filter_frame(host["mean"], host["variance"], host["position"], host["normal"], host["diffuse_albedo"], settings)
        assert not differing(host["out_colour"], want_colour).any() and not differing(host["out_variance"], want_variance).any()
        # it is a filter: the covered pixels changed, the others did not
        assert host["out_colour"][covered].tobytes() != host["mean"][covered].tobytes()
        assert host["out_colour"][~covered].tobytes() == host["mean"][~covered].tobytes()
    finally:
        r.close()
        for buffer in list(buffers.values()) + ring:
            buffer.free()


def test_radiance_target_between_frames_in_flight(dataset):
    """The radiance target itself as colour, queued between frames in flight: the filter reads frame 2 - not frame 1, not
    frame 3, which waits for it - and the frames are those of a run without the filter"""
    width, height = EXTENT
    shape, image_bytes = (height, width, 4), width * height * 16

    def run(with_filter):
        r = open_renderer(dataset, frames_in_flight=3)
        names = ("position", "normal", "diffuse_albedo", "out_colour")
        buffers = {name: DeviceBuffer(image_bytes) for name in names}
        radiance, filtered, host = [], None, None
        try:
            features = {name: buffers[name].ptr.value for name in names[:3]}
            # (in both runs: with animated noise every upload of the constants, this call's too, takes the next seed)
            r.render_features(list(features), pointers=features)
            r.render()
            r.render()
            if with_filter:
                assert r.filter_frame(r.app.render_targets.radiance, None, features, FRAME_SETTINGS, out_colour=buffers["out_colour"].ptr.value) is None
            else:
                radiance.append(r.read_radiance())
            r.render()
            radiance.append(r.read_radiance())
            r.render()
            radiance.append(r.read_radiance())
            if with_filter:
                r.sync()
                host = {name: buffers[name].download(shape, np.float32) for name in names}
        finally:
            r.close()
            for buffer in buffers.values():
                buffer.free()
        return radiance, host

    with_filter, host = run(True)
    without = run(False)[0]
    second, third, fourth = without
    assert second.tobytes() != third.tobytes() and np.isfinite(second).all() and second[..., :3].max() > 0
    assert with_filter[0].tobytes() == third.tobytes() and with_filter[1].tobytes() == fourth.tobytes()
    want = frame_filter.filter_frame(second, None, host["position"], host["normal"], host["diffuse_albedo"], FRAME_SETTINGS)[0]
    assert not differing(host["out_colour"], want).any()
    assert differing(want, frame_filter.filter_frame(third, None, host["position"], host["normal"], host["diffuse_albedo"], FRAME_SETTINGS)[0]).any()


def test_arithmetic_mode_of_the_pass_changes_nothing(dataset):
    """The filter is one build in one arithmetic: under a pass of any mode the same inputs give the same bytes, numpy's; the
    filter has another extent (40x24) than the swapchain (16x16)"""
    name = "non_finite"
    width, height = cases.CASES[name][:2]
    images = cases.inputs(name)
    want_colour, want_variance, _ = cases.expected(name, 5)
    features = {"position": images["position"], "normal": images["normal"]}
    for arithmetic in ("libm", "exact", "fast"):
        r = open_renderer(dataset, arithmetic, extent=(16, 16))
        try:
            r.render()
            filter_ = r.create_frame_filter(width, height)
            assert (filter_.width, filter_.height) == (width, height) != (16, 16)
            got_colour, got_variance = r.filter_frame(images["colour"], images["variance"], features, cases.settings(name, 5), frame_filter=filter_)
            assert got_colour.tobytes() == want_colour.tobytes() and got_variance.tobytes() == want_variance.tobytes(), arithmetic
        finally:
            r.close()


# ---- 3. the object and the refusals ------------------------------------------------------------------------------------------

def test_create_and_destroy_twice(device):
    lib = capi.load()
    e = device.app.swapchain.extent
    kept = (e.width, e.height)
    try:
        e.width, e.height = 33, 35
        images = cases.inputs("33x35")
        want = cases.expected("33x35", 5)[0]
        features = {"position": images["position"], "normal": images["normal"]}
        for _ in range(2):
            # (0, 0: the swapchain extent)
            filter_ = device.create_frame_filter()
            assert (filter_.width, filter_.height) == (33, 35) and filter_.filter.filtered and filter_.filter.colour_scratch[1] and filter_.filter.variance_scratch[1]
            assert device.filter_frame(images["colour"], images["variance"], features, cases.settings("33x35"), frame_filter=filter_)[0].tobytes() == want.tobytes()
            filter_.close()
            assert not filter_.filter.filtered and not filter_.filter.colour_scratch[0] and filter_.filter.width == 0
            # destroying what is destroyed does nothing
            lib.destroy_frame_filter(C.byref(filter_.filter), C.byref(device.app))
    finally:
        e.width, e.height = kept


def test_refusals_write_nothing(device, capfd):
    name = "16x16"
    width, height = cases.CASES[name][:2]
    arena = FilterArena(width, height, cases.inputs(name))
    filter_ = device.create_frame_filter(width, height)
    lib = capi.load()
    good = cases.settings(name, 2)
    nan = float("nan")

    def refused(settings=None, change=None, filter_struct=None):
        images = arena.images()
        if change:
            change(images)
        flush_c_output()
        capfd.readouterr()
        result = lib.filter_frame(C.byref(filter_struct if filter_struct is not None else filter_.filter), C.byref(device.app),
                                  C.byref(settings_struct(dict(good, **(settings or {})))), C.byref(images))
        flush_c_output()
        printed = capfd.readouterr().out
        assert result == 1 and printed.count("\n") == 1 and printed.endswith("\n"), (settings, printed)
        device.sync()
        assert arena.untouched(), (settings, printed)

    def set_member(member, value):
        return lambda images: setattr(images, member, value)
    try:
        for settings in [dict(iteration_count=0), dict(iteration_count=6), dict(normal_squarings=9), dict(sigma_luminance=0.0), dict(sigma_luminance=nan),
                         dict(sigma_depth=-1.0), dict(sigma_depth=float("inf")), dict(variance_scale=-1.0), dict(variance_scale=nan)]:
            refused(settings)
        for member in ("colour", "position", "normal", "out_colour"):
            refused(change=set_member(member, None))
        for member, _ in capi.FrameFilterImages._fields_:
            refused(change=lambda images, member=member: setattr(images, member, getattr(images, member) + 4))
        refused(change=set_member("variance", None))
        # an output that overlaps an input - the same image, or its last pixel - or the other output
        for member in ("colour", "variance", "position", "normal", "modulation"):
            refused(change=lambda images, member=member: setattr(images, "out_colour", getattr(images, member)))
            refused(change=lambda images, member=member: setattr(images, "out_variance", getattr(images, member) + arena.image_bytes - 16))
        refused(change=lambda images: setattr(images, "out_variance", images.out_colour))
        refused(change=lambda images: setattr(images, "out_variance", images.out_colour - arena.image_bytes + 16))
        # a filter that was not created, or no longer is
        refused(filter_struct=capi.FrameFilter())
        gone = device.create_frame_filter(width, height)
        gone.close()
        refused(filter_struct=gone.filter)
        # (the same request is accepted once nothing is wrong with it)
        assert lib.filter_frame(C.byref(filter_.filter), C.byref(device.app), C.byref(settings_struct(good)), C.byref(arena.images())) == 0
        device.sync()
        got_colour, got_variance, guards_intact = arena.read()
        want_colour, want_variance, _ = cases.expected(name, 2)
        assert guards_intact and got_colour.tobytes() == want_colour.tobytes() and got_variance.tobytes() == want_variance.tobytes()
    finally:
        filter_.close()
        arena.free()


# ---- 4. the command line -----------------------------------------------------------------------------------------------------

def test_command_line_writes_the_noisy_and_the_filtered_image(dataset, tmp_path):
    """python -m vulkan_renderer_amd.frame_filter, called in this process, at 83x45: its files are those of the same calls
    made here"""
    width, height = EXTENT
    root = os.path.dirname(dataset["scene"])
    arguments = [root, "--width", str(width), "--height", str(height), "--spp", "1", "--frames", "3", "--iterations", "3"]
    assert frame_filter.main(arguments + ["--out", str(tmp_path / "hdr"), "--hdr"]) == 0
    assert frame_filter.main(arguments + ["--out", str(tmp_path / "png"), "--png"]) == 0
    image_bytes = width * height * 16
    names = ("mean", "variance", "position", "normal", "diffuse_albedo", "filtered", "encoded")
    buffers = {name: DeviceBuffer(image_bytes) for name in names}
    r = renderer.Renderer()
    try:
        renderer.setup_config(r, 3, dataset, width, height, sample_count=1, acceleration_structure=True)
        r.app.render_settings.animate_noise = 1
        r.create_targets()
        r.create_pass()
        r.render_visibility()
        statistics = r.create_statistics(width * height)
        for _ in range(3):
            r.render()
            statistics.accumulate()
        statistics.resolve(buffers["mean"].ptr.value, buffers["variance"].ptr.value)
        features = {name: buffers[name].ptr.value for name in ("position", "normal", "diffuse_albedo")}
        r.render_features(list(features), pointers=features)
        settings = dict(frame_filter.DEFAULT_SETTINGS, iteration_count=3, variance_scale=1.0 / 3)
        r.filter_frame(buffers["mean"].ptr.value, buffers["variance"].ptr.value, features, settings, out_colour=buffers["filtered"].ptr.value)
        for name, key in (("noisy", "mean"), ("filtered", "filtered")):
            assert open(tmp_path / "hdr" / (name + ".hdr"), "rb").read() == r.encode_hdr(buffers[key].ptr.value, width=width, height=height)
            r.encode_slab(buffers[key].ptr.value, buffers["encoded"].ptr.value, width * height)
            file = open(tmp_path / "png" / (name + ".png"), "rb").read()
            assert file == r.encode_png(buffers["encoded"].ptr.value, width=width, height=height)
            assert np.asarray(png_cases.decode(file)).size == width * height * 3
        assert open(tmp_path / "hdr" / "noisy.hdr", "rb").read() != open(tmp_path / "hdr" / "filtered.hdr", "rb").read()
    finally:
        r.close()
        for buffer in buffers.values():
            buffer.free()
