"""Radiance RGBE *.hdr files as include/vkr_hdr.h defines them, restated in numpy: every byte of the file that the device
encoder (csrc/hdr_encoder.hip) and the reference's writer (stbi_write_hdr at src/main.c:1757) produce.  The run-length
coding is the statement without a cursor of the header - stretches, runs, dumps, costs per element and their exclusive
sum - over all planes of the image at once.

    python -m vulkan_renderer_amd.hdr INPUT.npy OUTPUT.hdr [--through-half]

encodes an image on the device (float32, height x width x 3 or 4)."""
import re
import sys

import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max
HEADER = "#?RADIANCE\n# Written by stb_image_write.h\nFORMAT=32-bit_rle_rgbe\nEXPOSURE=          1.0000000000000\n\n-Y %d +X %d\n"


def header(width, height):
    return (HEADER % (height, width)).encode()


def run_length_coded(width):
    return 8 <= width < 32768


def capacity(width, height):
    """get_hdr_capacity() of include/vkr_hdr.h: a coded plane never exceeds width + ceil(width / 128) bytes"""
    if not (0 < width <= 65535 and 0 < height <= 65535):
        return 0
    if not run_length_coded(width):
        return len(header(width, height)) + 4 * width * height
    return len(header(width, height)) + height * (4 + 4 * (width + (width + 127) // 128))


def sanitise(image, through_half=False):
    """c >= 0 ? min(c, FLT_MAX) : 0 per channel; through_half: first to the nearest half and back"""
    c = np.asarray(image, F)
    if through_half:
        with np.errstate(over="ignore", invalid="ignore"):
            c = c.astype(np.float16).astype(F)
    with np.errstate(invalid="ignore"):
        return np.where(c >= 0, np.minimum(c, FLT_MAX), F(0)).astype(F)


def rgbe(image, through_half=False):
    """The RGBE bytes (height, width, 4) of a float image (height, width, 3 or 4)"""
    c = sanitise(np.asarray(image)[..., :3], through_half)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    inner = np.where(g > b, g, b)
    m = np.where(r > inner, r, inner)
    dark = m < F(1e-32)
    safe = np.where(dark, F(1), m)
    f, e = np.frexp(safe)
    normalize = (f.astype(F) * F(256.0)) / safe
    out = np.zeros(c.shape[:2] + (4,), np.uint8)
    for k in range(3):
        out[..., k] = (c[..., k] * normalize).astype(np.int64).astype(np.uint8)
    out[..., 3] = ((e.astype(np.int64) + 128) & 255).astype(np.uint8)
    out[dark] = 0
    return out


def shifted(mask, by, fill=False):
    """mask[:, i + by] at [:, i], `fill` where that is outside the row"""
    out = np.full_like(mask, fill)
    if by > 0 and by < mask.shape[1]:
        out[:, :-by] = mask[:, by:]
    elif by < 0 and -by < mask.shape[1]:
        out[:, -by:] = mask[:, :by]
    elif by == 0:
        out[:] = mask
    return out


def code_planes(planes):
    """Run-length codes every row of a uint8 array (count, width) on its own.  Returns (coded, sizes): a uint8 array
    (count, width + ceil(width / 128)) whose row n holds sizes[n] coded bytes."""
    planes = np.ascontiguousarray(planes, np.uint8)
    count, width = planes.shape
    index = np.arange(width, dtype=np.int64)[None, :]
    equal = np.zeros((count, width), bool)
    equal[:, 1:] = planes[:, 1:] == planes[:, :-1]
    e_before, e1, e2 = shifted(equal, -1), shifted(equal, 1), shifted(equal, 2)
    # part of three equal bytes as the last, the middle or the first of them
    run = (e_before & equal) | (equal & e1) | (e1 & e2)
    stretch_start = np.maximum.accumulate(np.where(~equal, index, 0), axis=1)
    dump_starts = ~run & shifted(run, -1, True)
    dump_start = np.maximum.accumulate(np.where(dump_starts, index, 0), axis=1)
    k = index - np.where(run, stretch_start, dump_start)
    cost = np.where(run, np.where(k % 127 == 0, 2, 0), 1 + (k % 128 == 0))
    inclusive = np.cumsum(cost, axis=1)
    at = inclusive - cost
    sizes = inclusive[:, -1]
    coded = np.zeros((count, width + (width + 127) // 128), np.uint8)
    rows = np.broadcast_to(np.arange(count)[:, None], (count, width))
    # runs: the last element of a packet writes {128 + n, value}
    j = k % 127
    last = run & ((j == 126) | ~e1)
    packet = np.where(j == 0, at, at - 2)
    coded[rows[last], packet[last]] = (129 + j[last]).astype(np.uint8)
    coded[rows[last], packet[last] + 1] = planes[last]
    # dumps: every element writes its byte, the last one of a packet the count in front of it
    j = k % 128
    data = at + (j == 0)
    dump = ~run
    coded[rows[dump], data[dump]] = planes[dump]
    last = dump & ((j == 127) | shifted(run, 1) | (index == width - 1))
    coded[rows[last], (data - j - 1)[last]] = (j[last] + 1).astype(np.uint8)
    return coded, sizes


def encode(image, through_half=False):
    """The bytes of the file of a float image (height, width, 3 or 4; a fourth channel is ignored)"""
    image = np.asarray(image)
    if image.ndim != 3 or image.shape[2] not in (3, 4) or image.shape[0] == 0 or image.shape[1] == 0:
        raise ValueError("an HDR file is made from a float image of shape (height, width, 3 or 4)")
    height, width = image.shape[:2]
    quadruples = rgbe(image, through_half)
    if not run_length_coded(width):
        return header(width, height) + quadruples.tobytes()
    scanline = bytes([2, 2, width >> 8, width & 255])
    pieces = [header(width, height)]
    # (64 rows at a time: the temporaries of code_planes() are sixteen times the planes)
    for first in range(0, height, 64):
        rows = quadruples[first:first + 64]
        # (row, plane) in file order
        coded, sizes = code_planes(rows.transpose(0, 2, 1).reshape(rows.shape[0] * 4, width))
        for n in range(len(sizes)):
            if n % 4 == 0:
                pieces.append(scanline)
            pieces.append(coded[n, :sizes[n]].tobytes())
    return b"".join(pieces)


def decode(data):
    """The RGBE bytes (height, width, 4) that a file holds"""
    match = re.search(rb"\n\n-Y (\d+) \+X (\d+)\n", data)
    if not data.startswith(b"#?RADIANCE\n") or not match:
        raise ValueError("not a Radiance file of the kind the writer makes")
    height, width = int(match.group(1)), int(match.group(2))
    at = match.end()
    if not run_length_coded(width):
        if len(data) != at + 4 * width * height:
            raise ValueError("%d bytes behind the header instead of %d" % (len(data) - at, 4 * width * height))
        return np.frombuffer(data, np.uint8, 4 * width * height, at).reshape(height, width, 4).copy()
    out = np.zeros((height, 4, width), np.uint8)
    for y in range(height):
        if data[at:at + 4] != bytes([2, 2, width >> 8, width & 255]):
            raise ValueError("row %d does not start with a scanline header" % y)
        at += 4
        for plane in range(4):
            x = 0
            while x < width:
                n = data[at]
                if n > 128:
                    n -= 128
                    out[y, plane, x:x + n] = data[at + 1]
                    at += 2
                else:
                    out[y, plane, x:x + n] = np.frombuffer(data, np.uint8, n, at + 1)
                    at += 1 + n
                if n == 0 or x + n > width:
                    raise ValueError("a packet of row %d leaves the row" % y)
                x += n
    if at != len(data):
        raise ValueError("%d bytes behind the last row" % (len(data) - at))
    return np.ascontiguousarray(out.transpose(0, 2, 1))


def main(argv):
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("input", help="*.npy (float32, height x width x 3 or 4)")
    ap.add_argument("output", help="the *.hdr to write")
    ap.add_argument("--through-half", action="store_true", help="round every channel to half precision first, as the screenshots do")
    args = ap.parse_args(argv)
    image = np.ascontiguousarray(np.load(args.input), F)
    from . import renderer
    r = renderer.Renderer()
    try:
        data = r.encode_hdr(image, through_half=args.through_half)
    finally:
        r.close()
    with open(args.output, "wb") as file:
        file.write(data)
    print("Wrote %s: %d x %d, %d bytes." % (args.output, image.shape[1], image.shape[0], len(data)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
