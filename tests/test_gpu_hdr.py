"""The Radiance encoder on the device (include/vkr_hdr.h, csrc/hdr_encoder.hip) against the numpy restatement
vulkan_renderer_amd/hdr.py and the files of the reference's writer (tests/golden/hdr.npz), which tests/test_hdr.py pins
to each other, and against that writer itself where oracle/_ref is present: every byte and the size, through RGB and
RGBA input and padded rows; values the writer is not defined on; raw and widest rows; the bounds of
encode_hdr_on_device(); slots on the frame streams; reuse and re-creation; the screenshot calls and the tools."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import golden_cases
import hdr_cases
from helpers import DeviceBuffer
from test_experiments import decode_hdr
from test_gpu_golden import render_case
from vulkan_renderer_amd import capi, convergence, experiments, hdr, renderer, synthetic

pytestmark = pytest.mark.gpu

F = np.float32
CASES = hdr_cases.cases()
SPECIALS = hdr_cases.special_inputs()


@pytest.fixture(scope="module")
def device():
    r = renderer.Renderer()
    yield r
    r.close()


def with_alpha(image, alpha=np.nan):
    """a fourth channel that must not matter"""
    return np.concatenate([image[..., :3], np.full(image.shape[:2] + (1,), alpha, F)], axis=-1)


def assert_same_file(got, expected, what):
    assert hdr_cases.first_difference(got, expected) is None, what


def test_the_library_states_the_sizes_of_the_rule(device):
    lib = device.lib
    assert lib.get_hdr_chunk_size() == hdr_cases.CHUNK and lib.get_hdr_segment_size() == hdr_cases.SEGMENT
    buffer = C.create_string_buffer(capi.HDR_MAX_HEADER_SIZE)
    for width, height in ((1, 1), (7, 2), (8, 1), (1920, 1080), (32767, 65535), (32768, 1), (65535, 65535)):
        assert lib.get_hdr_header(buffer, width, height) == len(hdr.header(width, height)) and buffer.value == hdr.header(width, height)
        assert lib.get_hdr_capacity(width, height) == hdr.capacity(width, height)
    assert lib.get_hdr_header(buffer, 0, 1) == 0 and lib.get_hdr_capacity(65536, 1) == 0


def check_all_layouts(device, name, image, through_half, expected):
    height, width = image.shape[:2]
    encoder = device.create_hdr_encoder(width, height)
    assert encoder.capacity == hdr.capacity(width, height) >= len(expected)
    rgb, rgba = np.ascontiguousarray(image[..., :3]), with_alpha(image)
    # RGB and RGBA (loaded as float4 where rows allow it), rows further apart than a row: by one float and by four
    for what, pixels, stride in (("rgb", rgb, 0), ("rgba", rgba, 0), ("rgb padded", rgb, 12 * width + 20), ("rgba padded, floats", rgba, 16 * width + 4),
                                 ("rgba padded, float4", rgba, 16 * width + 32)):
        assert_same_file(encoder.encode_image(pixels, stride, through_half), expected, (name, what))
    encoder.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_the_restatement_and_the_writers_file(device, name):
    image, through_half = CASES[name]
    expected = hdr_cases.restated(name)
    assert expected == hdr_cases.fixtures()[name][2]
    check_all_layouts(device, name, image, through_half, expected)


@pytest.mark.parametrize("name", sorted(SPECIALS))
def test_nan_inf_and_negative_inputs(device, name):
    image, through_half = SPECIALS[name]
    assert np.isnan(image).any() and np.isinf(image).any() and (image < 0).any()
    check_all_layouts(device, name, image, through_half, hdr_cases.restated(name))


def stretches(width, height, seed):
    """noise in which every fourth pixel or so starts a stretch of equal pixels, a few of them long"""
    rng = np.random.default_rng(seed)
    lengths = rng.choice([1, 1, 1, 2, 3, 5, 130, 300], (height, width))
    image = np.stack([np.repeat(hdr_cases.scaled_noise(width, 1, seed + y)[0], lengths[y], axis=0)[:width] for y in range(height)])
    return np.ascontiguousarray(image, F)


@pytest.mark.parametrize("width,height", [(32768, 1), (32767, 2), (2 * hdr_cases.SEGMENT, 3), (2 * hdr_cases.SEGMENT + 1, 1), (hdr_cases.SEGMENT - 1, 2)])
def test_the_widest_rows(device, width, height):
    """32768: the first width that is not run-length coded again; 32767: thirty-two segments of sixteen chunks per row"""
    image = stretches(width, height, width)
    expected = hdr.encode(image)
    got = device.encode_hdr(image)
    print("%d x %d: %d bytes of %d" % (width, height, len(got), hdr.capacity(width, height)))
    assert_same_file(got, expected, (width, height))
    if hdr_cases.reference_available():
        assert_same_file(got, hdr_cases.reference_file(image), "writer")


@pytest.mark.skipif(not hdr_cases.reference_available(), reason="oracle/_ref is not built")
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_the_live_writer(device, name):
    image, through_half = CASES[name]
    assert_same_file(device.encode_hdr(image, through_half), hdr_cases.reference_file(image, through_half), name)


@pytest.mark.parametrize("name", ["noise_257x1", "noise_7x2"])
def test_encode_on_device_stays_within_its_capacity(device, name):
    image, _ = CASES[name]
    expected = hdr_cases.restated(name)
    size = len(expected)
    encoder = device.create_hdr_encoder(image.shape[1], image.shape[0])
    pixels, guard = DeviceBuffer(image.nbytes), 256
    pixels.upload(image)
    out, size_word = DeviceBuffer(size + guard), DeviceBuffer(8)
    pattern = np.full(size + guard, 0xA5, np.uint8)
    for capacity in (size, size - 1, size - 2, 600, 100, 70, 1, 0, size + 7):
        out.upload(pattern)
        size_word.zero()
        encoder.encode_on_device(pixels.ptr, out.ptr, capacity, size_word.ptr, channel_count=3)
        device.sync()
        got = out.download(size + guard, np.uint8)
        written = min(capacity, size)
        assert int(size_word.download(1, np.uint64)[0]) == size, capacity
        assert got[:written].tobytes() == expected[:written], capacity
        assert (got[written:] == 0xA5).all(), capacity
    # the host path afterwards, through the same slot
    assert_same_file(encoder.encode(pixels.ptr, 3), expected, "host path")
    for buffer in (pixels, out, size_word):
        buffer.free()
    encoder.close()


def test_two_slots_on_the_frame_streams(dataset):
    width, height = 192, 108
    r = renderer.Renderer(frames_in_flight=3)
    renderer.setup_config(r, 3, dataset, width=width, height=height)
    r.create_targets()
    r.create_pass()
    r.render_visibility()
    r.render()
    encoder = r.create_hdr_encoder(width, height, slot_count=2)
    radiance = [DeviceBuffer(width * height * 16) for _ in range(3)]
    streams, files = [], []
    # three frames in flight, two slots: the third frame takes the slot of the first, whose file has been fetched
    for frame in range(3):
        r.app.render_settings.exposure_factor *= 0.5 + frame
        streams.append(r.next_frame_stream())
        r.render(radiance[frame].ptr.value)
        if frame == 2:
            files.append(encoder.end(0))
        encoder.begin(frame % 2, radiance[frame].ptr, 4, 0, stream=streams[frame])
    assert len(set(streams)) == 3 and all(s in [int(x) for x in r.app.device.frame_streams if x] for s in streams)
    files += [encoder.end(1), encoder.end(0)]
    r.sync()
    for frame in range(3):
        image = radiance[frame].download((height, width, 4), F)
        assert_same_file(files[frame], hdr.encode(image), frame)
    assert len(set(files)) == 3
    # a view of the staging memory instead of a copy; through the half
    encoder.begin(1, radiance[0].ptr, 4, 0, through_half=True)
    assert encoder.end(1, copy=False).tobytes() == hdr.encode(radiance[0].download((height, width, 4), F), True) != files[0]
    with pytest.raises(RuntimeError):
        encoder.begin(2, radiance[0].ptr, 4, 0)
    with pytest.raises(RuntimeError):
        encoder.begin(0, radiance[0].ptr, 2, 0)
    with pytest.raises(RuntimeError):
        encoder.begin(0, radiance[0].ptr, 4, 16 * width - 4)
    with pytest.raises(RuntimeError):
        encoder.begin(0, radiance[0].ptr, 4, 16 * width + 2)
    for buffer in radiance:
        buffer.free()
    r.close()
    assert encoder.closed


def test_an_encoder_is_reused_and_recreated(device):
    encoder = device.create_hdr_encoder(70, 5)
    files = []
    for round_ in range(20):
        image = stretches(70, 5, round_ % 10)
        files.append(encoder.encode_image(image))
        assert_same_file(files[-1], hdr.encode(image), round_)
    assert files[:10] == files[10:] and len(set(files)) == 10
    with pytest.raises(RuntimeError):
        encoder.end(1)
    encoder.close()
    encoder.close()
    # another extent, nine slots; the end of a slot that never began is refused
    encoder = device.create_hdr_encoder(33, 31, slot_count=9)
    image = stretches(33, 31, 4)
    assert_same_file(encoder.encode_image(image), hdr.encode(image), "recreated")
    with pytest.raises(RuntimeError):
        encoder.end(8)
    encoder.close()
    for width, height, slots in ((0, 5, 1), (5, 65536, 1), (5, 5, 0), (5, 5, 10)):
        with pytest.raises(RuntimeError):
            renderer.HdrEncoder(device, width, height, slots)
    zeroed = capi.HdrEncoder()
    assert device.lib.create_hdr_encoder(C.byref(zeroed), None, 5, 5, 1) == 1 and not zeroed.state and zeroed.width == 0


@pytest.fixture(scope="module")
def golden_dataset(tmp_path_factory):
    return synthetic.write_dataset(str(tmp_path_factory.mktemp("dataset")), **golden_cases.DATASET)


def test_hdr_screenshot_is_the_writers_file(golden_dataset, tmp_path):
    r, image = render_case(golden_cases.FRAME_CASES[3], golden_dataset, False, 200, 120)
    assert np.isfinite(image[..., :3]).all() and (image[..., :3] >= 0).all() and len(np.unique(image[..., :3])) > 50
    path, host_path = str(tmp_path / "shot.hdr"), str(tmp_path / "host.hdr")
    r.app.screenshot.frame_bits = 2
    assert r.lib.take_hdr_screenshot(C.byref(r.app), path.encode()) == 0
    assert r.app.screenshot.frame_bits == 2
    r.app.screenshot.frame_bits = 0
    assert r.lib.take_hdr_screenshot(C.byref(r.app), None) == 0
    got = open(path, "rb").read()
    assert_same_file(got, hdr.encode(image, True), "restatement")
    if hdr_cases.reference_available():
        assert_same_file(got, hdr_cases.reference_file(image, True), "writer")
    assert got == r.read_hdr(through_half=True) != r.read_hdr()
    # the host path that exists: other header text, the same rows
    assert r.lib.take_screenshot(C.byref(r.app), None, host_path.encode()) == 0
    host = open(host_path, "rb").read()
    assert got[:len(hdr.header(200, 120))] == hdr.header(200, 120)
    rows_at = host.index(b"\n", host.index(b"\n\n") + 2) + 1
    assert host[:rows_at] != hdr.header(200, 120) and host[rows_at:] == got[len(hdr.header(200, 120)):]
    # the reader of tests/test_experiments.py reads the device's file
    assert np.array_equal(decode_hdr(got), hdr.rgbe(image, True)) and np.array_equal(hdr.decode(got), decode_hdr(host))
    r.close()


def test_experiment_stores_a_device_hdr(tmp_path):
    root = str(tmp_path / "root")
    table = experiments.experiment_table()
    index = next(i for i in range(table.count) if table.experiments[i].screenshot_path == b"data/experiments/mis_plane_clamped_optimal_ours_2spp_%.3f.png")
    assert experiments.main(["-e", str(index), "--synthetic", root, "--frames", "2", "--device-hdr"]) == 0
    files = glob.glob(os.path.join(root, "data", "experiments", "mis_plane_clamped_optimal_ours_2spp_*.hdr"))
    assert len(files) == 1 and not glob.glob(os.path.join(root, "data", "experiments", "*.png"))
    data = open(files[0], "rb").read()
    assert data.startswith(hdr.header(1024, 1024)) and len(data) <= hdr.capacity(1024, 1024)
    quadruples = hdr.decode(data)
    assert quadruples.shape == (1024, 1024, 4) and len(np.unique(quadruples[..., 3])) > 2
    with pytest.raises(SystemExit):
        experiments.main(["-e", str(index), "--synthetic", root, "--jpg", "--device-hdr"])


def test_convergence_stores_the_mean_as_hdr(tmp_path, capsys):
    import json
    path = str(tmp_path / "mean.hdr")
    assert convergence.main(["--frames", "4", "--reference-frames", "0", "--width", "96", "--height", "54", "--mean-hdr", path]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    data = open(path, "rb").read()
    assert line["mean_hdr_bytes"] == len(data) and data.startswith(hdr.header(96, 54))
    quadruples = hdr.decode(data)
    assert quadruples.shape == (54, 96, 4) and quadruples[..., :3].max() > 127


def test_a_full_size_rendered_frame(dataset):
    r = renderer.Renderer()
    renderer.setup_config(r, 3, dataset, width=1920, height=1080)
    r.create_targets()
    r.create_pass()
    r.render_visibility()
    r.render()
    got = r.read_hdr()
    image = r.read_radiance()
    assert len(np.unique(image[..., :3])) > 1000
    print("1920 x 1080 frame: %d bytes of Radiance file for %d bytes of RGBA32F" % (len(got), image.nbytes))
    assert_same_file(got, hdr.encode(image), "frame")
    assert_same_file(r.read_hdr(through_half=True), hdr.encode(image, True), "frame through the half")
    r.close()
