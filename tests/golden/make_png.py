"""TEST INFRASTRUCTURE.  Generates tests/golden/png.npz from the reference's own PNG writer: stbi_write_png of
oracle/_ref/libref_host.so (the reference's vendored stb_image_write.h, compiled as oracle/Makefile.ref says), called
through oracle.reference.write_png as src/main.c:1738 calls it.  The images are the 30 golden frames of
tests/golden/frames.npz as the project encodes them to sRGB8 and the generated images of tests/png_cases.py.  Only the
writer's files are stored - PNG is lossless, so the tests decode them to get the images back -, nothing of the writer's
text.
Run from the repository root, after the oracle has been built:
    python tests/golden/make_png.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUTPUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "png.npz")


def main():
    import png_cases
    from vulkan_renderer_amd import png
    if not png_cases.reference_available():
        raise SystemExit("oracle/_ref is missing: build the oracle first.")
    arrays = {}
    images = {**png_cases.golden_frame_images(), **png_cases.generated_fixture_images()}
    for name, image in images.items():
        data = png_cases.reference_file(image)
        assert np.array_equal(png_cases.decode(data), image), name
        ours = png.encode(image)
        same_stream = png_cases.inflated_idat(ours)[2] == png_cases.inflated_idat(data)[2]
        print("%-34s %6d bytes, restatement %6d, filtered stream %s, filters %s" % (name, len(data), len(ours), "equal" if same_stream else "DIFFERS",
                                                                                 sorted(set(png_cases.filters_of(data).tolist()))))
        arrays[name] = np.frombuffer(data, np.uint8)
    np.savez(OUTPUT, **arrays)
    print("Wrote %s (%d bytes)." % (OUTPUT, os.path.getsize(OUTPUT)))


if __name__ == "__main__":
    main()
