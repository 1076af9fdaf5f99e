"""The JPEG encoder on the device (include/vkr_jpeg.h, csrc/jpeg_encoder.hip) against the numpy restatement
vulkan_renderer_amd/jpeg.py, which tests/test_jpeg.py pins to the reference's writer, and against that writer itself
where oracle/_ref is present: every byte and the size, through RGBA8 and packed RGB8 input and padded rows; a rendered
frame; the screenshot calls; the bounds of encode_jpeg_on_device(); slots on the frame streams; reuse and re-creation."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import golden_cases
import jpeg_cases
from helpers import DeviceBuffer
from test_gpu_golden import render_case
from vulkan_renderer_amd import experiments, jpeg, renderer, synthetic

pytestmark = pytest.mark.gpu

INPUTS = jpeg_cases.device_inputs()
with_reference = pytest.mark.skipif(not jpeg_cases.reference_available(), reason="oracle/_ref is not built")


@pytest.fixture(scope="module")
def device():
    r = renderer.Renderer()
    yield r
    r.close()


def with_alpha(image, alpha=77):
    return np.concatenate([image[..., :3], np.full(image.shape[:2] + (1,), alpha, np.uint8)], axis=-1)


def assert_same_file(got, expected, what):
    assert jpeg_cases.first_difference(got, expected) is None, what


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_device_equals_the_restatement(device, name):
    image, quality = INPUTS[name]
    expected, statistics = jpeg_cases.restated(name)
    encoder = device.create_jpeg_encoder(image.shape[1], image.shape[0], quality)
    assert encoder.capacity >= len(expected) and encoder.encoder.data_unit_count == statistics["data_units"]
    rgba, width = with_alpha(image), image.shape[1]
    # packed RGB8, RGBA8 (read as dwords), rows further apart than a row: odd strides (bytes) and an aligned one (dwords)
    for what, pixels, stride in (("rgb8", image, 0), ("rgba8", rgba, 0), ("rgb8 padded", image, 3 * width + 5), ("rgba8 padded, unaligned", rgba, 4 * width + 3),
                                 ("rgba8 padded, aligned", rgba, 4 * width + 12)):
        assert_same_file(encoder.encode_image(pixels, stride), expected, (name, what))
    encoder.close()


def test_the_chunked_noise_puts_0xff_bytes_on_the_borders_of_stuffing_chunks(device):
    chunk = device.lib.get_jpeg_stuffing_chunk_size()
    expected, statistics = jpeg_cases.restated("noise_256x144_q95")
    positions = statistics["stuffed_positions"]
    print("chunk", chunk, "bytes", len(expected), "chunks", -(-(statistics["bits"] // 8) // chunk), "stuffed", len(positions))
    assert statistics["bits"] // 8 > 100 * chunk
    # a 0xFF that closes a chunk (its zero opens the next lane's bytes) and one that opens a chunk
    assert (positions % chunk == chunk - 1).any() and (positions % chunk == 0).any()
    # more than one workgroup of 256 lanes in the length scan and in packing
    assert jpeg_cases.restated("noise_136x72_q70")[1]["data_units"] > 256


@with_reference
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_device_equals_the_writer(device, name):
    image, quality = INPUTS[name]
    assert_same_file(device.encode_jpeg(image, quality), jpeg_cases.reference_file(image, quality), name)
    assert_same_file(device.encode_jpeg(with_alpha(image), quality), jpeg_cases.reference_file(with_alpha(image), quality), name)


def test_a_rendered_frame(dataset):
    full_size = jpeg_cases.reference_available()
    width, height = (1920, 1080) if full_size else (256, 144)
    r = renderer.Renderer()
    renderer.setup_config(r, 3, dataset, width=width, height=height)
    r.create_targets()
    r.create_pass()
    r.render_visibility()
    r.render()
    got = r.read_jpeg()
    rgb = np.ascontiguousarray(r.read_encoded()[..., :3])
    assert len(np.unique(rgb)) > 50
    expected = jpeg_cases.reference_file(rgb, 70) if full_size else jpeg.encode(rgb, 70)[0]
    print("%d x %d frame: %d bytes of JPEG for %d bytes of RGBA8" % (width, height, len(got), width * height * 4))
    assert_same_file(got, expected, "frame")
    # another quality through the same call: another cached encoder
    other = r.read_jpeg(quality=92)
    assert other != got and other[:2] == b"\xFF\xD8" and other[-2:] == b"\xFF\xD9" and other[0x9A + 11] == 0x11
    r.close()


@pytest.fixture(scope="module")
def golden_dataset(tmp_path_factory):
    return synthetic.write_dataset(str(tmp_path_factory.mktemp("dataset")), **golden_cases.DATASET)


def test_jpg_screenshot_is_the_writers_file(golden_dataset, tmp_path):
    r, _ = render_case(golden_cases.FRAME_CASES[3], golden_dataset, False, 200, 120)
    path = str(tmp_path / "shot.jpg")
    r.app.screenshot.frame_bits = 2
    assert r.lib.take_jpg_screenshot(C.byref(r.app), path.encode()) == 0
    assert r.app.screenshot.frame_bits == 2
    r.app.screenshot.frame_bits = 0
    assert r.lib.take_jpg_screenshot(C.byref(r.app), None) == 0
    rgb = np.ascontiguousarray(r.read_encoded(False, 0)[..., :3])
    got = open(path, "rb").read()
    assert_same_file(got, jpeg.encode(rgb, 70)[0], "restatement")
    if jpeg_cases.reference_available():
        assert_same_file(got, jpeg_cases.reference_file(rgb, 70), "writer")
    r.close()


def test_experiment_stores_a_jpg(tmp_path):
    root = str(tmp_path / "root")
    table = experiments.experiment_table()
    index = next(i for i in range(table.count) if table.experiments[i].screenshot_path == b"data/experiments/mis_plane_clamped_optimal_ours_2spp_%.3f.png")
    assert experiments.main(["-e", str(index), "--synthetic", root, "--frames", "2", "--jpg"]) == 0
    jpgs = glob.glob(os.path.join(root, "data", "experiments", "mis_plane_clamped_optimal_ours_2spp_*.jpg"))
    pngs = glob.glob(os.path.join(root, "data", "experiments", "mis_plane_clamped_optimal_ours_2spp_*.png"))
    assert len(jpgs) == 1 and len(pngs) == 1 and jpgs[0][:-3] == pngs[0][:-3]
    data = open(jpgs[0], "rb").read()
    assert data[:607] == jpeg.header(1024, 1024, 70) and data[-2:] == b"\xFF\xD9" and len(data) > 607 + 2 + 64 * 64 * 6 // 2
    with pytest.raises(SystemExit):
        experiments.main(["-e", str(index), "--synthetic", root, "--jpg", "--hdr"])


def test_encode_on_device_stays_within_its_capacity(device):
    image, quality = INPUTS["noise_136x72_q70"]
    expected = jpeg_cases.restated("noise_136x72_q70")[0]
    size = len(expected)
    encoder = device.create_jpeg_encoder(image.shape[1], image.shape[0], quality)
    pixels, guard = DeviceBuffer(image.nbytes), 256
    pixels.upload(image)
    out, size_word = DeviceBuffer(size + guard), DeviceBuffer(8)
    pattern = np.full(size + guard, 0xA5, np.uint8)
    for capacity in (size, size - 1, size - 2, 1000, 100, 1, 0, size + 7):
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
    r = renderer.Renderer(frames_in_flight=2)
    renderer.setup_config(r, 3, dataset, width=width, height=height)
    r.create_targets()
    r.create_pass()
    r.render_visibility()
    r.render()
    encoder = r.create_jpeg_encoder(width, height, 70, slot_count=2)
    radiance = [DeviceBuffer(width * height * 16) for _ in range(2)]
    packed = [DeviceBuffer(width * height * 3) for _ in range(2)]
    streams = []
    for slot in range(2):
        r.app.render_settings.exposure_factor *= 0.5 + slot
        streams.append(r.next_frame_stream())
        r.render_encoded(radiance[slot].ptr.value, packed[slot].ptr.value)
        encoder.begin(slot, packed[slot].ptr, 3, 0, stream=streams[slot])
    assert streams[0] != streams[1] and all(s in [int(x) for x in r.app.device.frame_streams if x] for s in streams)
    files = [encoder.end(slot) for slot in range(2)]
    r.sync()
    for slot in range(2):
        rgb = packed[slot].download((height, width, 3), np.uint8)
        assert_same_file(files[slot], jpeg.encode(rgb, 70)[0], slot)
    assert files[0] != files[1]
    # a view of the staging memory instead of a copy
    encoder.begin(1, packed[0].ptr, 3, 0)
    assert encoder.end(1, copy=False).tobytes() == files[0]
    with pytest.raises(RuntimeError):
        encoder.begin(2, packed[0].ptr, 3, 0)
    with pytest.raises(RuntimeError):
        encoder.begin(0, packed[0].ptr, 2, 0)
    with pytest.raises(RuntimeError):
        encoder.begin(0, packed[0].ptr, 3, 3 * width - 1)
    for buffer in radiance + packed:
        buffer.free()
    r.close()
    assert encoder.closed


def test_an_encoder_is_reused_and_recreated(device):
    encoder = device.create_jpeg_encoder(40, 24, 70)
    first = None
    for seed in (1, 2, 3, 1):
        image = jpeg_cases.noise(40, 24, seed)
        got = encoder.encode_image(image)
        assert_same_file(got, jpeg.encode(image, 70)[0], seed)
        first = first or got
    assert got == first
    with pytest.raises(RuntimeError):
        encoder.end(1)
    encoder.close()
    encoder.close()
    # another extent and another quality, nine slots; the end of a slot that never began is refused
    encoder = device.create_jpeg_encoder(33, 31, 100, slot_count=9)
    image = jpeg_cases.noise(33, 31, 4)
    assert_same_file(encoder.encode_image(image), jpeg.encode(image, 100)[0], "recreated")
    with pytest.raises(RuntimeError):
        encoder.end(8)
    encoder.close()
    for width, height, slots in ((0, 5, 1), (5, 65536, 1), (5, 5, 0), (5, 5, 10)):
        with pytest.raises(RuntimeError):
            renderer.JpegEncoder(device, width, height, 70, slots)
