"""The JPEG, Radiance and PNG encoders side by side (csrc/output_slots.hip holds what they share: the slots, their staging
memory and their events): encoders of the three formats with two slots each, all six encodes in flight at once, fetched
in the reverse order; then two of the encoders outlive the third, and Renderer.close() closes what is left."""
import numpy as np
import pytest

from helpers import DeviceBuffer
from vulkan_renderer_amd import hdr, jpeg, png, renderer

pytestmark = pytest.mark.gpu

# the extent of the reuse tests: wider than a chunk of 64 of the Radiance rows, more than one column of JPEG MCUs
WIDTH, HEIGHT = 70, 5


def test_six_encodes_of_three_formats_in_flight():
    r = renderer.Renderer()
    rng = np.random.default_rng(22)
    bytes_image = lambda: rng.integers(0, 256, (HEIGHT, WIDTH, 3), dtype=np.uint8)
    images = {"jpeg": [bytes_image(), bytes_image()],
              "hdr": [rng.random((HEIGHT, WIDTH, 3), np.float32), rng.random((HEIGHT, WIDTH, 3), np.float32)],
              "png": [bytes_image(), bytes_image()]}
    expected = {"jpeg": [jpeg.encode(image)[0] for image in images["jpeg"]],
                "hdr": [hdr.encode(image) for image in images["hdr"]],
                "png": [png.encode(image) for image in images["png"]]}
    encoders = {"jpeg": r.create_jpeg_encoder(WIDTH, HEIGHT, slot_count=2), "hdr": r.create_hdr_encoder(WIDTH, HEIGHT, slot_count=2),
                "png": r.create_png_encoder(WIDTH, HEIGHT, slot_count=2)}
    pixels = {}
    for name in images:
        for slot, image in enumerate(images[name]):
            pixels[name, slot] = DeviceBuffer(image.nbytes)
            pixels[name, slot].upload(image)
    order = [(name, slot) for slot in range(2) for name in ("jpeg", "hdr", "png")]
    for name, slot in order:
        encoders[name].begin(slot, pixels[name, slot].ptr, 3, 0)
    files = {(name, slot): encoders[name].end(slot) for name, slot in reversed(order)}
    for name, slot in order:
        assert files[name, slot] == expected[name][slot], (name, slot)
    assert len(set(files.values())) == 6
    # two encoders outlive the third
    encoders["hdr"].close()
    for name in ("jpeg", "png"):
        for slot in range(2):
            assert encoders[name].encode(pixels[name, slot].ptr, 3) == expected[name][slot], (name, slot, "after closing the HDR encoder")
    for buffer in pixels.values():
        buffer.free()
    r.close()
    assert encoders["jpeg"].closed and encoders["hdr"].closed and encoders["png"].closed
