"""Baseline JPEG files as include/vkr_jpeg.h defines them, restated in numpy: every byte of the file that the device
encoder (csrc/jpeg_encoder.hip) and the reference's writer (stbi_write_jpg at src/main.c:1745-1752) produce.  All
arithmetic is binary32 with one rounding per operation, in the order the header gives.

    python -m vulkan_renderer_amd.jpeg INPUT.npy|INPUT.png OUTPUT.jpg [--quality Q]

encodes an image on the device (uint8, height x width x 3 or 4; *.png is read with PIL where it can be imported)."""
import sys

import numpy as np

F = np.float32
HEADER_SIZE = 607

# ITU-T T.81 Annex K: Table K.1 (luminance) and K.2 (chrominance) quantisation, row by row
K1 = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
               14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
               49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
K2 = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
               47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64)


# Tables K.3 - K.6: (codes per length 1 ... 16, symbols in order of increasing code length)
DC_LUMINANCE = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMINANCE = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMINANCE = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D],
                [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
                 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72,
                 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37,
                 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
                 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83,
                 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3,
                 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3,
                 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
                 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])
AC_CHROMINANCE = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
                  [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
                   0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1,
                   0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36,
                   0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
                   0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A,
                   0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A,
                   0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA,
                   0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
                   0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])
# the order of the DHT segment
HUFFMAN_SPECIFICATIONS = (DC_LUMINANCE, AC_LUMINANCE, DC_CHROMINANCE, AC_CHROMINANCE)
HUFFMAN_CLASS_AND_ID = (0x00, 0x10, 0x01, 0x11)

# the AAN scale factors
AAN = (1.0, 1.387039845, 1.306562965, 1.175875602, 1.0, 0.785694958, 0.541196100, 0.275899379)


def zigzag_positions():
    """position[n]: where coefficient n = 8 row + column stands in the zig-zag sequence (T.81 figure A.6)"""
    order = sorted(range(64), key=lambda n: (n // 8 + n % 8, n // 8 if (n // 8 + n % 8) % 2 else n % 8))
    position = np.zeros(64, np.int64)
    position[order] = np.arange(64)
    return position


ZIGZAG = zigzag_positions()


def huffman_codes(specification):
    """(code, length) per symbol, 256 entries, length 0 for a symbol without code: the canonical construction of T.81
    Annex C (figures C.1 - C.3) from the counts per length and the symbols in order"""
    counts, symbols = specification
    codes = np.zeros((256, 2), np.int64)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            codes[symbols[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    assert k == len(symbols)
    return codes


def effective_quality(quality):
    """(quality in 1 ... 100, 4:2:0 subsampling): 0 means 90, subsampling is decided before the clamp"""
    quality = int(quality) if quality else 90
    return min(max(quality, 1), 100), quality <= 90


def quantisation_tables(quality):
    """(luminance, chrominance) table entries in natural order for an effective quality"""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * s + 50) // 100, 1, 255) for base in (K1, K2))


def descaling_factors(table):
    """1.0f / ((entry * a[row]) * a[column]) with a[k] = AAN[k] * 2.828427125f, all binary32"""
    a = np.array([F(c) * F(2.828427125) for c in AAN], F)
    entry = table.astype(F).reshape(8, 8)
    return (F(1.0) / ((entry * a[:, None]) * a[None, :])).astype(F)


def header(width, height, quality):
    """The 607 bytes in front of the entropy-coded segment"""
    quality, subsampled = effective_quality(quality)
    out = bytearray([0xFF, 0xD8, 0xFF, 0xE0, 0, 16]) + b"JFIF\0" + bytearray([1, 1, 0, 0, 1, 0, 1, 0, 0])
    out += bytearray([0xFF, 0xDB, 0, 0x84])
    for index, table in enumerate(quantisation_tables(quality)):
        in_zigzag_order = np.zeros(64, np.uint8)
        in_zigzag_order[ZIGZAG] = table
        out += bytes([index]) + in_zigzag_order.tobytes()
    out += bytearray([0xFF, 0xC0, 0, 17, 8, height >> 8, height & 255, width >> 8, width & 255, 3,
                      1, 0x22 if subsampled else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
    out += bytearray([0xFF, 0xC4, 0x01, 0xA2])
    for class_and_id, (counts, symbols) in zip(HUFFMAN_CLASS_AND_ID, HUFFMAN_SPECIFICATIONS):
        out += bytes([class_and_id]) + bytes(counts) + bytes(symbols)
    out += bytearray([0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    assert len(out) == HEADER_SIZE
    return bytes(out)


def data_unit_count(width, height, quality):
    _, subsampled = effective_quality(quality)
    mcu = 16 if subsampled else 8
    return ((width + mcu - 1) // mcu) * ((height + mcu - 1) // mcu) * (6 if subsampled else 3)


def capacity(width, height, quality):
    """get_jpeg_capacity() of include/vkr_jpeg.h: the header, per data unit the longest DC code with its extra bits and
    63 times the longest AC code with its extra bits, one byte of fill, all of that doubled for stuffing, and EOI"""
    dc = max(int(length) + symbol for spec in (DC_LUMINANCE, DC_CHROMINANCE) for symbol, (_, length) in enumerate(huffman_codes(spec)) if length)
    ac = max(int(length) + (symbol & 15) for spec in (AC_LUMINANCE, AC_CHROMINANCE) for symbol, (_, length) in enumerate(huffman_codes(spec)) if length)
    bits = data_unit_count(width, height, quality) * (dc + 63 * ac)
    return HEADER_SIZE + 2 * ((bits + 7) // 8 + 1) + 2


def _dct(d):
    """One AAN pass over the eight arrays d[0] ... d[7]"""
    d0, d1, d2, d3, d4, d5, d6, d7 = d
    tmp0, tmp7, tmp1, tmp6 = d0 + d7, d0 - d7, d1 + d6, d1 - d6
    tmp2, tmp5, tmp3, tmp4 = d2 + d5, d2 - d5, d3 + d4, d3 - d4
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    o0, o4 = tmp10 + tmp11, tmp10 - tmp11
    z1 = (tmp12 + tmp13) * F(0.707106781)
    o2, o6 = tmp13 + z1, tmp13 - z1
    tmp10, tmp11, tmp12 = tmp4 + tmp5, tmp5 + tmp6, tmp6 + tmp7
    z5 = (tmp10 - tmp12) * F(0.382683433)
    z2 = tmp10 * F(0.541196100) + z5
    z4 = tmp12 * F(1.306562965) + z5
    z3 = tmp11 * F(0.707106781)
    z11, z13 = tmp7 + z3, tmp7 - z3
    return [o0, z11 + z4, o2, z13 - z2, o4, z13 + z2, o6, z11 - z4]


def _bit_length(magnitude):
    length = np.zeros(magnitude.shape, np.int64)
    rest = magnitude.copy()
    while rest.any():
        length += rest > 0
        rest >>= 1
    return length


def data_units(image, quality=70):
    """The quantised coefficients in scan order, (data units, 64) int32 in zig-zag order, and the component (0, 1, 2) of
    every data unit"""
    image = np.asarray(image)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] not in (3, 4) or image.shape[0] == 0 or image.shape[1] == 0:
        raise ValueError("a JPEG is made from a uint8 image of shape (height, width, 3 or 4)")
    height, width = image.shape[:2]
    quality, subsampled = effective_quality(quality)
    mcu = 16 if subsampled else 8
    mcus_x, mcus_y = (width + mcu - 1) // mcu, (height + mcu - 1) // mcu
    rows = np.minimum(np.arange(mcus_y * mcu), height - 1)
    columns = np.minimum(np.arange(mcus_x * mcu), width - 1)
    rgb = image[rows][:, columns, :3].astype(F)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    y = ((F(0.299) * r + F(0.587) * g) + F(0.114) * b) - F(128)
    u = ((F(-0.16874) * r - F(0.33126) * g) + F(0.5) * b)
    v = ((F(0.5) * r - F(0.41869) * g) - F(0.08131) * b)

    def blocks(plane, per_axis):
        # (mcus, per_axis^2 blocks in raster order, 8, 8)
        return plane.reshape(mcus_y, per_axis, 8, mcus_x, per_axis, 8).transpose(0, 3, 1, 4, 2, 5).reshape(mcus_y * mcus_x, per_axis * per_axis, 8, 8)

    if subsampled:
        def mean(plane):
            return (((plane[0::2, 0::2] + plane[0::2, 1::2]) + plane[1::2, 0::2]) + plane[1::2, 1::2]) * F(0.25)
        units = np.concatenate([blocks(y, 2), blocks(mean(u), 1), blocks(mean(v), 1)], axis=1)
        components = np.array([0, 0, 0, 0, 1, 2])
    else:
        units = np.concatenate([blocks(y, 1), blocks(u, 1), blocks(v, 1)], axis=1)
        components = np.array([0, 1, 2])
    component = np.tile(components, mcus_x * mcus_y)
    units = units.reshape(-1, 8, 8)
    # rows first, then columns
    units = np.stack(_dct([units[:, :, k] for k in range(8)]), axis=2)
    units = np.stack(_dct([units[:, k, :] for k in range(8)]), axis=1)
    tables = quantisation_tables(quality)
    factors = np.stack([descaling_factors(tables[0]), descaling_factors(tables[1]), descaling_factors(tables[1])])
    scaled = units * factors[component]
    rounded = np.where(scaled < 0, scaled - F(0.5), scaled + F(0.5)).astype(np.int32)  # truncation
    coefficients = np.zeros((units.shape[0], 64), np.int32)
    coefficients[:, ZIGZAG] = rounded.reshape(-1, 64)
    return coefficients, component


def entropy_code(coefficients, component):
    """The entropy-coded segment without stuffing: (bytes with the last one filled with ones, bit count, statistics)"""
    count = coefficients.shape[0]
    coefficients = coefficients.astype(np.int64)
    dc_codes = [huffman_codes(DC_LUMINANCE), huffman_codes(DC_CHROMINANCE), huffman_codes(DC_CHROMINANCE)]
    ac_codes = [huffman_codes(AC_LUMINANCE), huffman_codes(AC_CHROMINANCE), huffman_codes(AC_CHROMINANCE)]
    dc_codes, ac_codes = np.stack(dc_codes), np.stack(ac_codes)
    keys, values, lengths = [], [], []

    def items(key, value, length):
        keys.append(key); values.append(value.astype(np.int64)); lengths.append(length.astype(np.int64))

    def extra_bits(value, size):
        return np.where(value < 0, value - 1, value) & ((np.int64(1) << size) - 1)

    # DC: the difference to the previous data unit of the same component
    difference = np.zeros(count, np.int64)
    for c in range(3):
        of_component = np.nonzero(component == c)[0]
        dc = coefficients[of_component, 0]
        difference[of_component] = dc - np.concatenate([[0], dc[:-1]])
    unit = np.arange(count, dtype=np.int64)
    size = _bit_length(np.abs(difference))
    code = dc_codes[component, np.minimum(size, 255)]
    items(unit * 256 + 1, code[:, 0], code[:, 1])
    items(unit * 256 + 2, extra_bits(difference, size), size)
    # AC: runs of zeros in front of every nonzero coefficient
    of_unit, position = np.nonzero(coefficients[:, 1:])
    position = position + 1
    first = np.concatenate([[True], of_unit[1:] != of_unit[:-1]]) if of_unit.size else np.zeros(0, bool)
    previous = np.where(first, 0, np.concatenate([[0], position[:-1]]))
    run = position - previous - 1
    value = coefficients[of_unit, position]
    ac_size = _bit_length(np.abs(value))
    zrl_count = run >> 4
    zrl = ac_codes[component[of_unit], 0xF0]
    repeated = sum(np.where(zrl_count > k, zrl[:, 0] << (zrl[:, 1] * k), 0) for k in range(3))
    items(of_unit * 256 + position * 3, repeated, zrl[:, 1] * zrl_count)
    code = ac_codes[component[of_unit], ((run & 15) << 4) + ac_size]
    items(of_unit * 256 + position * 3 + 1, code[:, 0], code[:, 1])
    items(of_unit * 256 + position * 3 + 2, extra_bits(value, ac_size), ac_size)
    last = np.zeros(count, np.int64)
    np.maximum.at(last, of_unit, position)
    with_eob = np.nonzero(last != 63)[0]
    eob = ac_codes[component[with_eob], 0x00]
    items(with_eob * 256 + 64 * 3, eob[:, 0], eob[:, 1])

    keys, values, lengths = np.concatenate(keys), np.concatenate(values), np.concatenate(lengths)
    order = np.argsort(keys, kind="stable")
    values, lengths = values[order], lengths[order]
    bit_count = int(lengths.sum())
    starts = np.cumsum(lengths) - lengths
    item = np.repeat(np.arange(values.size), lengths)
    shift = lengths[item] - 1 - (np.arange(bit_count) - starts[item])
    bits = ((values[item] >> shift) & 1).astype(np.uint8)
    bits = np.concatenate([bits, np.ones(-bit_count % 8, np.uint8)])
    statistics = {
        "data_units": int(count),
        "zrl_codes": int(zrl_count.sum()),
        "double_zrl": int((zrl_count >= 2).sum()),
        "data_units_without_eob": int(count - with_eob.size),
        "data_units_all_ac_zero": int((last == 0).sum()),
        "zero_dc_differences": int((difference == 0).sum()),
        "largest_dc_category": int(size.max()),
        "largest_ac_category": int(ac_size.max()) if ac_size.size else 0,
        "bits": bit_count,
    }
    return np.packbits(bits), bit_count, statistics


def stuff(packed):
    """A zero byte behind every 0xFF byte"""
    return np.insert(packed, np.nonzero(packed == 0xFF)[0] + 1, 0)


def encode(image, quality=70):
    """-> (the bytes of the file, statistics).  statistics counts what the entropy coder met: data_units, zrl_codes,
    double_zrl (coefficients with 32 or more zeros in front), data_units_without_eob, data_units_all_ac_zero,
    zero_dc_differences, largest_dc_category, largest_ac_category, bits, stuffed_bytes, last_byte_stuffed,
    ends_aligned (no fill byte) and stuffed_positions (offsets of the 0xFF bytes in the segment before stuffing)"""
    image = np.asarray(image)
    coefficients, component = data_units(image, quality)
    packed, bit_count, statistics = entropy_code(coefficients, component)
    positions = np.nonzero(packed == 0xFF)[0]
    statistics.update({"stuffed_bytes": int(positions.size), "last_byte_stuffed": bool(packed[-1] == 0xFF),
                       "ends_aligned": bit_count % 8 == 0, "stuffed_positions": positions})
    return header(image.shape[1], image.shape[0], quality) + stuff(packed).tobytes() + b"\xFF\xD9", statistics


def main(argv):
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("input", help="*.npy (uint8, height x width x 3 or 4) or an image PIL reads")
    ap.add_argument("output", help="the *.jpg to write")
    ap.add_argument("--quality", type=int, default=70)
    args = ap.parse_args(argv)
    if args.input.endswith(".npy"):
        image = np.load(args.input)
    else:
        try:
            from PIL import Image
        except ImportError:
            raise SystemExit("%s is not a .npy file and PIL cannot be imported." % args.input)
        image = np.asarray(Image.open(args.input).convert("RGB"))
    from . import renderer
    r = renderer.Renderer()
    try:
        data = r.encode_jpeg(np.ascontiguousarray(image, np.uint8), quality=args.quality)
    finally:
        r.close()
    with open(args.output, "wb") as file:
        file.write(data)
    print("Wrote %s: %d x %d, quality %d, %d bytes." % (args.output, image.shape[1], image.shape[0], args.quality, len(data)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
