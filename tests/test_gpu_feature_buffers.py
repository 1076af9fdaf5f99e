"""Feature buffers (include/vkr_feature_buffers.h) on the device: every image against the CPU oracle's shading data and the
numpy rules of vulkan_renderer_amd/feature_buffers.py, bit for bit in the libm and the polynomial mode; subsets, independence
of the frames of the pass, moved geometry, the fast mode against libm, the previews and the refusals.  The frames and what
they are chosen for: tests/feature_buffer_cases.py (the conditions are asserted there on the oracle's side, and without a
GPU in tests/test_feature_buffers.py)."""
import ctypes as C

import numpy as np
import pytest

import feature_buffer_cases as cases
import png_cases
from helpers import DeviceBuffer
from vulkan_renderer_amd import capi, feature_buffers, renderer, scene_update, synthetic

pytestmark = pytest.mark.gpu

ALL = capi.PIXEL_FEATURES
FRAMES = {"83x45": (83, 45), "16x16": (16, 16), "7x3": (7, 3), "textured_83x45": (83, 45)}
UNTEXTURED = ("83x45", "16x16", "7x3")
GUARD_BYTE, GUARD_BYTES = 0xA5, 256

# Fast mode against libm on the device: the largest absolute difference per image over the three untextured frames (channels
# x, y, z, w together), measured on an MI355X (profiles/r29_summary.md).  The frames are few and what the fast mode costs
# depends on the geometry - these look along the ground from 5 mm above it - so the test allows four times as much.
FAST_MEASURED = {
    "position": 1.717e-5,       # (16x16; 83x45 1.9e-6, 7x3 4.8e-7)
    "normal": 3.725e-7,         # (83x45)
    "outgoing": 3.248e-6,       # (83x45)
    "diffuse_albedo": 0.0,      # the same operations in both modes: a constant material and one product
    "fresnel_0": 0.0,
    "reprojection": 2.738,      # (83x45: X of a point next to the second camera's plane c_3 = 0; 16x16 2.2e-5, 7x3 4.8e-7)
}


@pytest.fixture(scope="module")
def datasets(dataset, tmp_path_factory):
    textured = synthetic.write_dataset(str(tmp_path_factory.mktemp("feature_textured")), **cases.TEXTURED_DATASET)
    return {key: textured if key.startswith("textured") else dataset for key in FRAMES}


def open_renderer(datasets, key, arithmetic="libm", **arguments):
    """A renderer with targets, pass and visibility of frame `key`"""
    r = renderer.Renderer(arithmetic=arithmetic, **arguments)
    width, height = FRAMES[key]
    cases.apply_frame(r, datasets[key], width, height, cases.TEXTURED_CAMERA if key.startswith("textured") else cases.CAMERA)
    r.create_targets()
    r.create_pass()
    r.render_visibility()
    return r


_rendered = {}


def rendered(datasets, key, arithmetic):
    """-> dict: the seven images of the device with the second camera's reprojection, the visibility, and (IEEE modes) what
    the oracle and the numpy rules make of the same frame; rendered once per module, left unchanged"""
    if (key, arithmetic) not in _rendered:
        r = open_renderer(datasets, key, arithmetic)
        try:
            second = cases.second_matrix(r)
            result = {"images": r.render_features(ALL, second), "visibility": r.read_visibility(), "second": second}
            if arithmetic != "fast":
                images, data, inputs, frame = cases.expected(r, result["visibility"], renderer.ORACLE_MATH_MODE[arithmetic], second)
                result.update(expected=images, data=data, inputs=inputs, frame=frame)
        finally:
            r.close()
        for image in result["images"].values():
            image.setflags(write=False)
        _rendered[(key, arithmetic)] = result
    return _rendered[(key, arithmetic)]


def bits(image):
    return np.ascontiguousarray(image).view(np.uint32)


# ---- 1. the IEEE modes against the oracle ------------------------------------------------------------------------------

@pytest.mark.parametrize("key", list(FRAMES))
@pytest.mark.parametrize("arithmetic", ["libm", "exact"])
def test_images_equal_the_oracle_in_every_bit(datasets, key, arithmetic):
    result = rendered(datasets, key, arithmetic)
    extent = FRAMES[key]
    if key.startswith("textured"):
        assert len(cases.tap_counts(result["frame"], result["inputs"])) >= 3
        cases.assert_frame_conditions(result["expected"], result["data"], result["inputs"], (0, 0))
    else:
        cases.assert_frame_conditions(result["expected"], result["data"], result["inputs"], extent, result["second"])
    assert set(result["images"]) == set(ALL)
    for name in ALL:
        got, expected = result["images"][name], result["expected"][name]
        assert got.shape == (extent[1], extent[0], 4) and got.dtype == expected.dtype
        different = (bits(got) != bits(expected)).any(axis=-1)
        print(key, arithmetic, name, "pixels that differ:", int(different.sum()))
        assert not different.any(), (name, np.argwhere(different)[:4].tolist(), got[different][:2], expected[different][:2])


# ---- 2. subsets ------------------------------------------------------------------------------------------------------

def test_one_image_at_a_time_and_nothing_else_is_written(datasets):
    key = "83x45"
    together = rendered(datasets, key, "libm")
    width, height = FRAMES[key]
    image_bytes = width * height * 16
    stride = GUARD_BYTES + image_bytes
    # [guard][image 0][guard][image 1] ... [guard]: every image has a guard on both sides
    arena = DeviceBuffer(len(ALL) * stride + GUARD_BYTES)
    # an image that another call has written: must stay as that call left it
    other = DeviceBuffer(image_bytes)
    r = open_renderer(datasets, key)
    try:
        r.render_features(["normal"], pointers={"normal": other.ptr.value})
        r.sync()
        for index, name in enumerate(ALL):
            arena.upload(np.full(arena.nbytes, GUARD_BYTE, np.uint8))
            address = arena.ptr.value + GUARD_BYTES + index * stride
            assert r.render_features([name], together["second"], pointers={name: address}) is None
            r.sync()
            after = arena.download((arena.nbytes,), np.uint8)
            first = GUARD_BYTES + index * stride
            assert after[first:first + image_bytes].tobytes() == together["images"][name].tobytes(), name
            assert (after[:first] == GUARD_BYTE).all() and (after[first + image_bytes:] == GUARD_BYTE).all(), name
            assert other.download((image_bytes,), np.uint8).tobytes() == together["images"]["normal"].tobytes(), name
    finally:
        r.close()
        arena.free()
        other.free()


# ---- 3. independence of the pass --------------------------------------------------------------------------------------

def test_feature_calls_leave_the_frames_alone(datasets):
    key = "83x45"

    def run(with_features):
        r = open_renderer(datasets, key, frames_in_flight=3)
        features, frames = [], []
        try:
            def take():
                if with_features:
                    features.append(r.render_features(ALL))
            take()  # before any frame
            r.render()
            frames.append(r.read_radiance())
            take()  # after one
            r.render()
            if with_features:
                # between two frames in flight: queued without waiting for them
                kept = {name: DeviceBuffer(FRAMES[key][0] * FRAMES[key][1] * 16) for name in ALL}
                r.render_features(ALL, pointers={name: buffer.ptr.value for name, buffer in kept.items()})
            r.render()
            frames.append(r.read_radiance())
            if with_features:
                r.sync()
                features.append({name: buffer.download((FRAMES[key][1], FRAMES[key][0], 4), np.uint32 if name == "identity" else np.float32) for name, buffer in kept.items()})
                for buffer in kept.values():
                    buffer.free()
        finally:
            r.close()
        return features, frames

    features, frames_with = run(True)
    _, frames_without = run(False)
    assert len(features) == 3
    for later in features[1:]:
        for name in ALL:
            assert later[name].tobytes() == features[0][name].tobytes(), name
    # (this call's matrix is the frame's own: every covered pixel comes back to itself)
    covered = features[0]["identity"][..., 0] != 0xFFFFFFFF
    assert (features[0]["reprojection"][..., 3][covered] == 1).all()
    for a, b in zip(frames_with, frames_without):
        assert a.tobytes() == b.tobytes() and np.isfinite(a).all() and a[..., :3].max() > 0


# ---- 4. moved geometry ------------------------------------------------------------------------------------------------

def test_images_follow_update_geometry(datasets):
    key = "83x45"
    r = open_renderer(datasets, key)
    try:
        before = r.render_features(["position"])["position"]
        words = r.host_inputs()["quantized_positions"]
        codes = scene_update.unpack_positions(words).astype(np.int64).reshape(-1, 3, 3)
        # every triangle as a whole by up to 2000 codes per axis (2 cm: the box is 20 m and 2^21 codes across)
        shift = np.random.default_rng(29).integers(-2000, 2001, (len(codes), 1, 3))
        moved = scene_update.pack_positions(np.clip(codes + shift, 0, scene_update.CODE_MAX).astype(np.uint32).reshape(-1, 3))
        assert not r.update_geometry(moved, policy="refit")["rebuilt"]
        r.render_visibility()
        got = r.render_features(ALL, cases.second_matrix(r))
        expected, data, inputs, _ = cases.expected(r, r.read_visibility(), 0, cases.second_matrix(r))
        assert np.array_equal(inputs["quantized_positions"], moved)
    finally:
        r.close()
    assert (bits(before) != bits(got["position"])).any()
    for name in ALL:
        assert got[name].tobytes() == expected[name].tobytes(), name


# ---- 5. the fast mode --------------------------------------------------------------------------------------------------

def test_fast_mode_stays_near_libm(datasets):
    largest = {name: 0.0 for name in FAST_MEASURED}
    for key in UNTEXTURED:
        fast, libm = rendered(datasets, key, "fast")["images"], rendered(datasets, key, "libm")["images"]
        covered = libm["identity"][..., 0] != 0xFFFFFFFF
        assert fast["identity"].tobytes() == libm["identity"].tobytes()
        for name in FAST_MEASURED:
            assert np.isfinite(fast[name][covered]).all(), name
            assert bits(fast[name])[~covered].tobytes() == bits(libm[name])[~covered].tobytes(), name
            difference = float(np.abs(fast[name][covered].astype(np.float64) - libm[name][covered].astype(np.float64)).max())
            print(key, name, "largest difference of the fast mode from libm: %.3e" % difference)
            largest[name] = max(largest[name], difference)
    print("over the frames:", {name: "%.3e" % value for name, value in largest.items()})
    for name, value in largest.items():
        assert value <= 4.0 * FAST_MEASURED[name], (name, value)


# ---- 6. previews -------------------------------------------------------------------------------------------------------

PREVIEW_RANGE = {"position": (0.5, 9.0), "reprojection": (0.0, 12.0)}


@pytest.mark.parametrize("key", ["83x45", "textured_83x45"])
def test_previews_equal_the_numpy_rules_and_survive_the_png_encoder(datasets, key):
    images = rendered(datasets, key, "libm")["images"]
    width, height = FRAMES[key]
    r = open_renderer(datasets, key)
    on_device = DeviceBuffer(width * height * 4)
    try:
        for name in ALL:
            value_range = PREVIEW_RANGE.get(name, (0.0, 1.0))
            expected = feature_buffers.preview(name, images[name], value_range)
            got = r.feature_preview(name, images[name], value_range)
            assert got.shape == (height, width, 4) and got.tobytes() == expected.tobytes(), (name, np.argwhere((got != expected).any(axis=-1))[:4].tolist())
            assert len(np.unique(expected[..., :3])) > 4, name
        # the preview left on the device goes to the PNG encoder as it is
        source = DeviceBuffer(width * height * 16)
        source.upload(images["normal"])
        assert r.feature_preview("normal", source.ptr.value, out_pointer=on_device.ptr.value) is None
        file = r.encode_png(on_device.ptr.value)
        source.free()
        decoded = np.asarray(png_cases.decode(file)).reshape(height, width, 3)
        assert decoded.tobytes() == feature_buffers.preview("normal", images["normal"])[..., :3].tobytes()
    finally:
        on_device.free()
        r.close()


def test_command_line_writes_arrays_and_previews(datasets, tmp_path):
    """python -m vulkan_renderer_amd.feature_buffers, called in this process: the arrays of --npy are the images of
    render_features() for the same frame, the file of --png decodes to the numpy preview of that image"""
    import os
    root = os.path.dirname(datasets["16x16"]["scene"])
    arguments = [root, "--config", "3", "--width", "16", "--height", "16", "--feature", "normal", "--feature", "identity"]
    assert feature_buffers.main(arguments + ["--npy", str(tmp_path / "npy")]) == 0
    assert feature_buffers.main(arguments + ["--png", str(tmp_path / "png")]) == 0
    r = renderer.Renderer()
    try:
        renderer.setup_config(r, 3, datasets["16x16"], 16, 16, acceleration_structure=True)
        r.create_targets()
        r.create_pass()
        r.render_visibility()
        images = r.render_features(["normal", "identity"])
    finally:
        r.close()
    for name in ("normal", "identity"):
        assert np.load(tmp_path / "npy" / (name + ".npy")).tobytes() == images[name].tobytes()
        decoded = np.asarray(png_cases.decode(open(tmp_path / "png" / (name + ".png"), "rb").read())).reshape(16, 16, 3)
        assert decoded.tobytes() == feature_buffers.preview(name, images[name], (0.0, 16.0))[..., :3].tobytes()
    assert (images["identity"][..., 0] != 0xFFFFFFFF).any()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------

def test_refusals_write_nothing(datasets):
    key = "16x16"
    width, height = FRAMES[key]
    image_bytes = width * height * 16
    guard = np.full(image_bytes + 64, GUARD_BYTE, np.uint8)
    target = DeviceBuffer(guard.nbytes)
    target.upload(guard)
    lib = capi.load()

    def request(address, index=0):
        buffers = capi.FeatureBuffers()
        buffers.images[index] = address
        for i in range(4):
            buffers.reprojection_matrix[i][i] = 1.0
        return buffers

    def refused(r, buffers):
        assert lib.render_feature_buffers(C.byref(r.app), C.byref(buffers)) == 1
        r.sync()
        assert target.download(guard.shape, np.uint8).tobytes() == guard.tobytes()

    try:
        # no pass; a pass but no targets
        r = renderer.Renderer()
        cases.apply_frame(r, datasets[key], width, height)
        refused(r, request(target.ptr.value))
        r.create_pass()
        refused(r, request(target.ptr.value))
        r.close()
        r = open_renderer(datasets, key)
        try:
            refused(r, capi.FeatureBuffers())
            refused(r, request(target.ptr.value + 4))
            refused(r, request(target.ptr.value + 8, index=5))
            r.set_tiles(tile_size=16, rank=0, rank_count=2)
            refused(r, request(target.ptr.value))
            r.set_tiles(tile_size=16, rank=0, rank_count=1, slab_layout=True)
            refused(r, request(target.ptr.value))
            r.set_tiles(tile_size=0, rank=0, rank_count=1, slab_layout=False)
            # (the same request is accepted once nothing is wrong with it)
            assert lib.render_feature_buffers(C.byref(r.app), C.byref(request(target.ptr.value))) == 0
            r.sync()
            written = target.download(guard.shape, np.uint8)
            assert (written[image_bytes:] == GUARD_BYTE).all() and written[:image_bytes].tobytes() != guard[:image_bytes].tobytes()
            # previews: no pixel_feature_t, an empty or undefined range where it is used, missing or misaligned pointers
            source = DeviceBuffer(image_bytes)
            target.upload(guard)
            app = C.byref(r.app)
            nan = float("nan")
            for arguments in [(len(ALL), source.ptr.value, target.ptr.value, 0.0, 1.0), (99, source.ptr.value, target.ptr.value, 0.0, 1.0),
                              (0xFFFFFFFF, source.ptr.value, target.ptr.value, 0.0, 1.0),
                              (0, source.ptr.value, target.ptr.value, 1.0, 1.0), (0, source.ptr.value, target.ptr.value, 2.0, 1.0),
                              (0, source.ptr.value, target.ptr.value, nan, 1.0), (6, source.ptr.value, target.ptr.value, 0.0, nan),
                              (6, source.ptr.value, target.ptr.value, 3.0, 3.0),
                              (1, None, target.ptr.value, 0.0, 1.0), (1, source.ptr.value, None, 0.0, 1.0),
                              (1, source.ptr.value + 4, target.ptr.value, 0.0, 1.0), (1, source.ptr.value, target.ptr.value + 2, 0.0, 1.0)]:
                assert lib.encode_feature_preview(app, *arguments) == 1, arguments
            r.sync()
            assert target.download(guard.shape, np.uint8).tobytes() == guard.tobytes()
            # (a range that the feature does not use is not looked at)
            assert lib.encode_feature_preview(app, 1, source.ptr.value, target.ptr.value, 1.0, 1.0) == 0
            r.sync()
            source.free()
        finally:
            r.close()
    finally:
        target.free()
