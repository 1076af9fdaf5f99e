"""TEST INFRASTRUCTURE.  Generates tests/golden/hdr.npz from the reference's own Radiance writer: stbi_write_hdr of
oracle/_ref/libref_host.so (the reference's vendored stb_image_write.h, compiled as oracle/Makefile.ref says), called
through oracle.reference.write_hdr as src/main.c:1757 calls it.  For each case of tests/hdr_cases.py the input image
(ours), whether it goes through the half first, and the bytes of the writer's file are stored.  Only data is stored:
nothing of the writer's text.
Run from the repository root, after the oracle has been built:
    python tests/golden/make_hdr.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUTPUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hdr.npz")


def main():
    import hdr_cases
    from vulkan_renderer_amd import hdr
    if not hdr_cases.reference_available():
        raise SystemExit("oracle/_ref is missing: build the oracle first.")
    arrays = {}
    for name, (image, through_half) in hdr_cases.cases().items():
        data = hdr_cases.reference_file(image, through_half)
        ours = hdr.encode(image, through_half)
        height, width = image.shape[:2]
        print("%-34s %7d bytes of %7d  restatement %s" % (name, len(data), hdr.capacity(width, height), "equal" if ours == data else "DIFFERS"))
        arrays[name + "/image"] = image
        arrays[name + "/through_half"] = np.bool_(through_half)
        arrays[name + "/file"] = np.frombuffer(data, np.uint8)
    np.savez_compressed(OUTPUT, **arrays)
    print("Wrote %s (%d bytes)." % (OUTPUT, os.path.getsize(OUTPUT)))


if __name__ == "__main__":
    main()
