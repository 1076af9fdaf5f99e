"""TEST INFRASTRUCTURE.  Generates tests/golden/jpeg.npz from the reference's own JPEG writer: stbi_write_jpg of
oracle/_ref/libref_host.so (the reference's vendored stb_image_write.h, compiled as oracle/Makefile.ref says), called
through ctypes as src/main.c:1745-1752 calls it.  For each case the input image (ours) and the bytes of the writer's file
are stored.  Only data is stored: nothing of the writer's text.
Run from the repository root, after the oracle has been built:
    python tests/golden/make_jpeg.py"""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

OUTPUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg.npz")


def noise(width, height, seed):
    return np.random.default_rng(seed).integers(0, 256, (height, width, 3), dtype=np.uint8)


def ramp(width, height):
    y, x = np.mgrid[0:height, 0:width]
    return np.stack([(x * 255) // max(width - 1, 1), (y * 255) // max(height - 1, 1), ((x + y) * 255) // max(width + height - 2, 1)], axis=-1).astype(np.uint8)


def checkerboard(width, height, square):
    y, x = np.mgrid[0:height, 0:width]
    return np.repeat((((x // square + y // square) % 2) * 255).astype(np.uint8)[..., None], 3, axis=-1)


def sparse(width, height, seed):
    """A smooth ramp with sparse high-frequency detail: some 8 x 8 blocks get one of the highest-frequency cosine
    patterns added, so that their last coefficients stand behind runs of 32 and more zeros"""
    image = ramp(width, height).astype(np.float64)
    rng = np.random.default_rng(seed)
    k = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    for by in range(0, height - 7, 8):
        for bx in range(0, width - 7, 8):
            if rng.integers(0, 3) == 0:
                image[by:by + 8, bx:bx + 8] += (rng.integers(30, 90) * np.outer(k, k))[..., None]
    return np.clip(np.rint(image), 0, 255).astype(np.uint8)


def stripes(width, height):
    """1-pixel black and white columns in the upper half, rows in the lower one"""
    y, x = np.mgrid[0:height, 0:width]
    return np.repeat((np.where(y < height // 2, x % 2, y % 2) * 255).astype(np.uint8)[..., None], 3, axis=-1)


def cases():
    """name -> (image, quality): the fixture set of tests/test_jpeg.py"""
    return {
        "pixel_q70": (noise(1, 1, 1), 70),
        "noise_16x16_q70": (noise(16, 16, 2), 70),
        "ramp_17x9_q70": (ramp(17, 9), 70),
        "ramp_33x31_q70": (ramp(33, 31), 70),
        "noise_136x72_q70": (noise(136, 72, 3), 70),
        "noise_40x24_q95": (noise(40, 24, 4), 95),
        "noise_40x24_q100": (noise(40, 24, 4), 100),
        "checkerboard_32x32_q100": (checkerboard(32, 32, 8), 100),
        "sparse_136x72_q70": (sparse(136, 72, 5), 70),
        "white_24x24_q100": (np.full((24, 24, 3), 255, np.uint8), 100),
        "noise_32x16_q1": (noise(32, 16, 6), 1),
        "stripes_32x32_q100": (stripes(32, 32), 100),
    }


def reference_file(image, quality, library=None):
    """The file stbi_write_jpg(path, w, h, 3 or 4, pixels, quality) writes"""
    from oracle import reference
    library = library or reference.host()
    library.stbi_write_jpg.restype = C.c_int
    library.stbi_write_jpg.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    image = np.ascontiguousarray(image, np.uint8)
    with tempfile.TemporaryDirectory() as directory:
        path = os.path.join(directory, "reference.jpg")
        assert library.stbi_write_jpg(path.encode(), image.shape[1], image.shape[0], image.shape[2], image.ctypes.data, int(quality)) == 1
        with open(path, "rb") as file:
            return file.read()


def main():
    from oracle import reference
    from vulkan_renderer_amd import jpeg
    if not reference.available():
        raise SystemExit("oracle/_ref is missing: build the oracle first.")
    arrays = {}
    for name, (image, quality) in cases().items():
        data = reference_file(image, quality)
        ours, statistics = jpeg.encode(image, quality)
        print("%-26s %6d bytes  restatement %s  %s" % (name, len(data), "equal" if ours == data else "DIFFERS",
                                                       {k: v for k, v in statistics.items() if k != "stuffed_positions"}))
        arrays[name + "/image"] = image
        arrays[name + "/quality"] = np.int32(quality)
        arrays[name + "/file"] = np.frombuffer(data, np.uint8)
    np.savez_compressed(OUTPUT, **arrays)
    print("Wrote %s (%d bytes)." % (OUTPUT, os.path.getsize(OUTPUT)))


if __name__ == "__main__":
    main()
