"""TEST INFRASTRUCTURE: the inputs that tests/test_hdr.py and tests/test_gpu_hdr.py share - float images of our own,
chosen so that every branch of the rule of include/vkr_hdr.h is the only thing that can explain a difference -, the
fixtures of tests/golden/hdr.npz (the files the reference's writer made of them, tests/golden/make_hdr.py) and the
reference's writer itself where oracle/_ref is present."""
import functools
import os
import tempfile

import numpy as np

from vulkan_renderer_amd import hdr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hdr.npz")
# VKR_HDR_CHUNK and VKR_HDR_SEGMENT of include/vkr_hdr.h (tests/test_gpu_hdr.py asserts that the library says the same)
CHUNK, SEGMENT = 64, 1024
F = np.float32
FLT_MAX = np.finfo(np.float32).max
WIDTHS = (1, 7, 8, 9, 127, 128, 129, 130, 131, 255, 256, 257, 385)
# (one to four rows each; the fixture file pays twelve bytes per pixel of noise)
ROWS = (1, 2, 3, 4, 1, 2, 1, 1, 3, 1, 2, 1, 4)


def from_bytes(red, blue=None):
    """An image (rows, width, 3) whose R and B planes are the given bytes (rows, width): the green channel 0.75 keeps the
    largest channel in [0.5, 1), so that the bytes are 256 times the values, G is 192 and E is 128 everywhere"""
    red = np.atleast_2d(np.asarray(red, np.uint8))
    blue = red[:, ::-1] if blue is None else np.atleast_2d(np.asarray(blue, np.uint8))
    image = np.full(red.shape + (3,), 0.75, F)
    image[..., 0] = red.astype(F) / F(256)
    image[..., 2] = blue.astype(F) / F(256)
    return image


def background(width):
    """bytes without two equal neighbours"""
    return (10 + np.arange(width) % 2).astype(np.uint8)


def placed(width, length, starts, value=200):
    row = background(width)
    for start in starts:
        assert 0 <= start and start + length <= width and (row[max(start - 1, 0):start + length + 1] < 100).all(), (start, length)
        row[start:start + length] = value
    return row


def scaled_noise(width, height, seed):
    """random floats, every pixel scaled by a power of ten of its own now and then: all four planes vary"""
    rng = np.random.default_rng(seed)
    image = rng.random((height, width, 3), F)
    scale = np.where(rng.random((height, width, 1)) < 0.2, 10.0 ** rng.integers(-30, 30, (height, width, 1)), 1.0)
    return (image * scale).astype(F)


def edge_values():
    tiny = F(1e-32)
    values = [tiny, np.nextafter(tiny, F(0)), np.nextafter(tiny, F(1)), F(0.99e-32), F(0), FLT_MAX, np.nextafter(FLT_MAX, F(0))]
    for k in (-100, -20, -1, 0, 1, 7, 8, 9, 100, 127):
        power = F(2.0) ** F(k)
        values += [power, np.nextafter(power, F(0)), np.nextafter(power, F(np.inf))]
        if k < 119:
            values.append(F(255.9999) * power)
    values = np.array(values, F)
    # every value as the largest channel of a pixel, next to channels a little and much smaller
    image = np.zeros((2, len(values), 3), F)
    image[0, :, 0] = values
    image[0, :, 1] = values * F(0.999)
    image[0, :, 2] = values * F(1.0 / 300.0)
    image[1, :, 2] = values[::-1]
    image[1, :, 0] = values[::-1] * F(0.5)
    return image


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (image, through_half): what the writer, the restatement and the device are held to"""
    out = {}
    for n, (width, height) in enumerate(zip(WIDTHS, ROWS)):
        out["noise_%dx%d" % (width, height)] = (scaled_noise(width, height, 100 + n), False)
    # no plane has a run: pairs of equal bytes in R, G and B, and an exponent that changes every two pixels as well
    pairs = (np.arange(256) // 2 % 2).astype(F)
    image = np.stack([(128 + np.arange(256) // 2) / 256.0, (192 + pairs) / 256.0, (250 - pairs * 7) / 256.0], axis=-1).astype(F)[None]
    out["no_runs_256x1"] = (image * (1 + pairs)[None, :, None], False)
    out["constant_300x2"] = (np.full((2, 300, 3), 0.5, F), False)
    # runs (2: a stretch too short for one) that start or end on the row's borders, on a multiple of the chunk and of the
    # segment, and that straddle one
    width = SEGMENT + 9 * CHUNK
    rows = []
    for length in (2, 3, 127, 128, 254):
        rows.append(placed(width, length, (0, 8 * CHUNK - length, SEGMENT, width - length)))
        rows.append(placed(width, length, (2 * CHUNK, SEGMENT - length, SEGMENT + CHUNK - 1)))
    out["placed_runs_%dx%d" % (width, len(rows))] = (from_bytes(np.stack(rows)), False)
    # dumps of exactly 128 and 129 bytes between runs
    row = np.concatenate([np.full(5, 200), background(128), np.full(5, 201), background(129), np.full(4, 202)]).astype(np.uint8)
    out["dumps_128_129_%dx1" % len(row)] = (from_bytes(row), False)
    out["run_in_the_last_three_50x1"] = (from_bytes(placed(50, 3, (47,))), False)
    out["two_equal_at_the_end_50x1"] = (from_bytes(placed(50, 2, (48,))), False)
    edges = edge_values()
    out["edge_values_%dx2" % edges.shape[1]] = (edges, False)
    out["edge_values_raw_7x2"] = (np.ascontiguousarray(edges[:, 3:10]), False)
    rng = np.random.default_rng(7)
    halves = (rng.random((2, 140, 3)) * 10.0 ** rng.integers(-6, 5, (2, 140, 1))).astype(np.float16).astype(F)
    out["halves_140x2"] = (halves, True)
    # floats that the half rounds, up to the largest half, and underflow to its subnormals and to zero
    out["through_half_140x2"] = ((rng.random((2, 140, 3)) * 10.0 ** rng.integers(-9, 5, (2, 140, 1))).astype(F), True)
    return out


def special_inputs():
    """name -> (image, through_half): values the writer is not defined on; the rule sanitises them"""
    rng = np.random.default_rng(8)
    image = rng.random((3, 70, 4), F)
    specials = np.array([np.nan, -1.0, -0.0, np.inf, -np.inf, -1e-40, 1e-40, 70000.0, 65520.0, 65519.0], F)
    image[rng.random(image.shape) < 0.3] = 0
    where = rng.random(image.shape) < 0.25
    image[where] = rng.choice(specials, int(where.sum()))
    # whole pixels of one special value too
    for n, value in enumerate(specials):
        image[0, 5 * n, :] = value
    return {"specials_70x3": (image, False), "specials_through_half_70x3": (image, True)}


@functools.lru_cache(maxsize=None)
def restated(name):
    image, through_half = {**cases(), **special_inputs()}[name]
    return hdr.encode(image, through_half)


@functools.lru_cache(maxsize=None)
def fixtures():
    """name -> (image, through_half, the writer's file as bytes)"""
    with np.load(GOLDEN) as archive:
        names = sorted({key.split("/")[0] for key in archive.files})
        return {name: (archive[name + "/image"], bool(archive[name + "/through_half"]), archive[name + "/file"].tobytes()) for name in names}


def reference_available():
    from oracle import reference
    return reference.available()


def writer_input(image, through_half=False):
    """The floats the reference hands to its writer: RGB, through the half where the frame took that way (the two
    frame_bits passes of the screenshot)"""
    rgb = np.ascontiguousarray(np.asarray(image, F)[..., :3])
    return rgb.astype(np.float16).astype(F) if through_half else rgb


def reference_file(image, through_half=False):
    """The file stbi_write_hdr of the reference writes (oracle.reference.write_hdr, as src/main.c:1757 calls it)"""
    from oracle import reference
    with tempfile.TemporaryDirectory() as directory:
        path = os.path.join(directory, "reference.hdr")
        reference.write_hdr(path, writer_input(image, through_half))
        with open(path, "rb") as file:
            return file.read()


def first_difference(a, b):
    """for assertion messages: where two files differ first"""
    if a == b:
        return None
    n = min(len(a), len(b))
    at = next((i for i in range(n) if a[i] != b[i]), n)
    return {"sizes": (len(a), len(b)), "first_difference": at, "got": a[at:at + 8].hex(), "expected": b[at:at + 8].hex()}
