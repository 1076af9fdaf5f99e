"""TEST INFRASTRUCTURE.  Generates tests/golden/texture_conversion.npz from the reference's texture converter
(tools/texture_conversion/main.c), compiled as it is into a temporary directory: for every input image the array the
tool read and every *.vkt file it wrote, as bytes.  The inputs are written with the project's own PNG and Radiance
writers (csrc/host/image_writers.c); for a *.hdr input the stored array holds the floats the tool's loader makes of the
RGBE bytes, m * 2^(e - 136).  Besides, the blocks the tool makes of flat grey images of every byte value.  Only data is
stored: nothing of the reference's text or binaries.
Run from the repository root after the library has been built:
    python tests/golden/make_texture_conversion.py [--reference /root/reference]"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from vulkan_renderer_amd import capi, synthetic  # noqa: E402


def byte_images():
    """name: (uint8 RGB image, formats)"""
    base, specular, normal = synthetic.procedural_textures(64, 3)
    rng = np.random.default_rng(2024)
    y, x = np.mgrid[0:64, 0:64] / 64.0
    smooth = np.stack([0.5 + 0.25 * np.sin(2.0 * np.pi * (x + 2.0 * y) + c) + 0.15 * np.sin(2.0 * np.pi * 3.0 * x - c)
                       + 0.08 * np.sin(2.0 * np.pi * 5.0 * y + 2.0 * c) for c in (0.0, 1.0, 2.0)], -1)
    smooth = np.clip(np.rint((smooth + rng.normal(0.0, 0.03, smooth.shape)) * 255.0), 0, 255).astype(np.uint8)
    random = lambda w, h: rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return {
        "base": (base, (131, 132)), "specular": (specular, (131,)), "normal": (normal, (141,)),
        "smooth": (smooth, (131, 132, 141)), "random": (random(64, 64), (131, 132, 141)),
        "wide": (random(64, 16), (131, 141)), "tall": (random(16, 64), (132, 141)),
        "tiny": (random(4, 4), (131, 132, 141)), "single": (random(1, 1), (131, 132, 141)),
    }


def float_images():
    """name: (float32 RGB image, formats): values across many binades, some below the halves' normal range and one row
    above their largest"""
    rng = np.random.default_rng(99)
    images = {}
    for name, (w, h) in (("probe", (32, 32)), ("strip", (32, 8))):
        image = (rng.random((h, w, 3)) * np.exp2(rng.integers(-6, 5, (h, w, 1)))).astype(np.float32)
        image[1, :8] *= 1.0e-6
        image[2, 8:16] *= 3.0e4
        image[3, 4:12] = 0.0
        images[name] = (image, (90, 97, 106, 109))
    return images


def read_hdr(path):
    """The floats stb_image's loader makes of a Radiance file written by write_hdr_rgb32f (run-length coded rows for
    widths 8 ... 32767, flat RGBE otherwise)"""
    data = open(path, "rb").read()
    end = data.index(b"\n\n") + 2
    line_end = data.index(b"\n", end)
    tokens = data[end:line_end].split()
    height, width = int(tokens[1]), int(tokens[3])
    cursor = line_end + 1
    rgbe = np.zeros((height, width, 4), np.uint8)
    for row in range(height):
        if width < 8 or width >= 32768:
            rgbe[row] = np.frombuffer(data, np.uint8, 4 * width, cursor).reshape(width, 4)
            cursor += 4 * width
            continue
        assert data[cursor] == 2 and data[cursor + 1] == 2 and (data[cursor + 2] << 8 | data[cursor + 3]) == width
        cursor += 4
        for c in range(4):
            x = 0
            while x < width:
                count = data[cursor]
                if count > 128:
                    rgbe[row, x:x + count - 128, c] = data[cursor + 1]
                    x += count - 128
                    cursor += 2
                else:
                    rgbe[row, x:x + count, c] = np.frombuffer(data, np.uint8, count, cursor + 1)
                    x += count
                    cursor += 1 + count
    scale = np.ldexp(np.float32(1.0), rgbe[..., 3:].astype(np.int32) - 136).astype(np.float32)
    return np.where(rgbe[..., 3:] == 0, np.float32(0.0), rgbe[..., :3].astype(np.float32) * scale).astype(np.float32)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--reference", default="/root/reference")
    arguments = parser.parse_args()
    lib = capi.load()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        tool = os.path.join(tmp, "texture_conversion")
        subprocess.check_call(["gcc", "-O2", os.path.join(arguments.reference, "tools", "texture_conversion", "main.c"), "-lm", "-o", tool])
        cases = []
        for name, (image, formats) in byte_images().items():
            path = os.path.join(tmp, name + ".png")
            image = np.ascontiguousarray(image)
            assert lib.write_png_rgb8(path.encode(), image.shape[1], image.shape[0], image.ctypes.data) == 0
            cases.append((name, path, image, formats))
        for name, (image, formats) in float_images().items():
            path = os.path.join(tmp, name + ".hdr")
            image = np.ascontiguousarray(image)
            assert lib.write_hdr_rgb32f(path.encode(), image.shape[1], image.shape[0], image.ctypes.data) == 0
            cases.append((name, path, read_hdr(path), formats))
        for name, path, image, formats in cases:
            out["input_" + name] = image
            for vk_format in formats:
                target = os.path.join(tmp, "%s_%d.vkt" % (name, vk_format))
                subprocess.check_call([tool, str(vk_format), path, target], stdout=subprocess.DEVNULL)
                out["vkt_%s_%d" % (name, vk_format)] = np.frombuffer(open(target, "rb").read(), np.uint8)
        # flat grey images, one per byte value.  4x4 as BC1 UNORM: the texels of level 0 are the bytes themselves, so
        # flat_blocks_131[g] is the block the tool makes of sixteen texels (g, g, g).  16x16 as BC1 sRGB: three levels
        # through the sRGB table, the filter and the sRGB quantisation, 16 + 4 + 1 blocks per grey level
        for vk_format, size in ((131, 4), (132, 16)):
            payloads = []
            for grey in range(256):
                path, target = os.path.join(tmp, "flat.png"), os.path.join(tmp, "flat.vkt")
                image = np.full((size, size, 3), grey, np.uint8)
                assert lib.write_png_rgb8(path.encode(), size, size, image.ctypes.data) == 0
                subprocess.check_call([tool, str(vk_format), path, target], stdout=subprocess.DEVNULL)
                data = open(target, "rb").read()
                level_count = int.from_bytes(data[8:12], "little")
                payloads.append(np.frombuffer(data[32 + 24 * level_count:-4], np.uint8).reshape(-1, 8))
            out["flat_blocks_%d" % vk_format] = np.stack(payloads)
    target = os.path.join(ROOT, "tests", "golden", "texture_conversion.npz")
    np.savez_compressed(target, **out)
    print("wrote %s: %d arrays, %d bytes" % (target, len(out), os.path.getsize(target)))


if __name__ == "__main__":
    main()
