"""TEST INFRASTRUCTURE: the inputs that tests/test_jpeg.py and tests/test_gpu_jpeg.py share - the fixtures of
tests/golden/jpeg.npz (images and the files the reference's writer made of them), generated inputs, and the reference's
writer itself where oracle/_ref is present."""
import ctypes as C
import functools
import os

import numpy as np

from vulkan_renderer_amd import jpeg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg.npz")


@functools.lru_cache(maxsize=None)
def fixtures():
    """name -> (image, quality, the writer's file as bytes)"""
    with np.load(GOLDEN) as archive:
        names = sorted({key.split("/")[0] for key in archive.files})
        return {name: (archive[name + "/image"], int(archive[name + "/quality"]), archive[name + "/file"].tobytes()) for name in names}


def noise(width, height, seed):
    return np.random.default_rng(seed).integers(0, 256, (height, width, 3), dtype=np.uint8)


# 256 x 144 noise at quality 95: a packed stream of many stuffing chunks.  The seed is the first one whose stream has a
# 0xFF byte as the last byte of a chunk of 64 and one as the first byte (tests/test_gpu_jpeg.py asserts both).
CHUNKED_NOISE_SEED = 1


@functools.lru_cache(maxsize=None)
def restated(name):
    """(file, statistics) of the restatement for a named input of device_inputs()"""
    image, quality = device_inputs()[name]
    return jpeg.encode(image, quality)


@functools.lru_cache(maxsize=None)
def device_inputs():
    """name -> (image, quality): what the device is held to"""
    golden = fixtures()
    inputs = {name: golden[name][:2] for name in ("pixel_q70", "noise_16x16_q70", "ramp_17x9_q70", "noise_136x72_q70", "sparse_136x72_q70",
                                                  "checkerboard_32x32_q100", "stripes_32x32_q100")}
    inputs["noise_8x8_q100"] = (noise(8, 8, 7), 100)
    inputs["noise_256x144_q95"] = (noise(256, 144, CHUNKED_NOISE_SEED), 95)
    return inputs


def reference_available():
    from oracle import reference
    return reference.available()


def reference_file(image, quality):
    """The file stbi_write_jpg(path, w, h, channels, pixels, quality) of the reference writes, as src/main.c:1745 calls it,
    collected in memory through stbi_write_jpg_to_func"""
    from oracle import reference
    library = reference.host()
    callback_type = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int)
    library.stbi_write_jpg_to_func.restype = C.c_int
    library.stbi_write_jpg_to_func.argtypes = [callback_type, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    image = np.ascontiguousarray(image, np.uint8)
    pieces = []
    callback = callback_type(lambda context, data, size: pieces.append(C.string_at(data, size)))
    assert library.stbi_write_jpg_to_func(callback, None, image.shape[1], image.shape[0], image.shape[2], image.ctypes.data, int(quality)) == 1
    return b"".join(pieces)


def first_difference(a, b):
    """for assertion messages: where two files differ first"""
    if a == b:
        return None
    n = min(len(a), len(b))
    at = next((i for i in range(n) if a[i] != b[i]), n)
    return {"sizes": (len(a), len(b)), "first_difference": at, "got": a[at:at + 8].hex(), "expected": b[at:at + 8].hex()}
