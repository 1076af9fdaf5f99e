"""PNG files as include/vkr_png.h defines them, restated in numpy: every byte of the file that the device encoder
(csrc/png_encoder.hip) produces.  The filtered stream is the one of the reference's writer (stbi_write_png at
src/main.c:1738) and of write_png_rgb8(); the deflate stream is this project's own: one block per segment, matches at three
fixed distances, dynamic Huffman codes where they are shorter than the fixed code.

    python -m vulkan_renderer_amd.png INPUT.npy OUTPUT.png

encodes an image on the device (uint8, height x width x 3 or 4)."""
import struct
import sys
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
UNIT = 4096           # VKR_PNG_UNIT
SEGMENT_BYTES = 65536  # VKR_PNG_SEGMENT_BYTES
MAX_MATCH = 258
LENGTH_BASE = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258])
LENGTH_EXTRA = np.array([0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0])
DISTANCE_BASE = np.array([1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577])
DISTANCE_EXTRA = np.array([0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13])
CODE_LENGTH_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LITERAL_COUNT, DISTANCE_COUNT = 286, 30
# the fixed code of RFC 1951 3.2.6: 288 literal and length symbols take part in it, 286 of them occur
FIXED_LITERAL_LENGTHS = np.array([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DISTANCE_LENGTHS = np.array([5] * 30)


def valid_extent(width, height):
    return 0 < width <= 65535 and 0 < height <= 65535


def rows_per_segment(row_length, rows):
    return max(1, min(SEGMENT_BYTES // row_length, rows))


def stream_capacity(row_length, rows):
    """CAPACITY of include/vkr_png.h for a filtered stream of `rows` rows of row_length bytes"""
    per_segment = rows_per_segment(row_length, rows)
    segments = (rows + per_segment - 1) // per_segment
    last_rows = rows - (segments - 1) * per_segment
    full, last = per_segment * row_length, last_rows * row_length
    return 8 + 25 + 12 + 2 + (segments - 1) * ((9 * full + 20) // 8 + 16) + (9 * last + 20) // 8 + 16


def capacity(width, height):
    """get_png_capacity()"""
    return stream_capacity(3 * width + 1, height) if valid_extent(width, height) else 0


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def header(width, height):
    """Signature and IHDR: the 33 bytes in front of the first IDAT"""
    return SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, 2, 0, 0, 0))


def filtered_stream(image):
    """F of the rule: (height, 1 + 3 width) bytes, per row the filter byte and the residuals of the filter with the
    smallest sum of |signed residual|, ties to the lower filter number"""
    image = np.asarray(image)
    if image.ndim != 3 or image.shape[2] not in (3, 4) or image.dtype != np.uint8 or 0 in image.shape:
        raise ValueError("a PNG file is made from a uint8 image of shape (height, width, 3 or 4)")
    height, width = image.shape[:2]
    raw = image[..., :3].reshape(height, 3 * width).astype(np.int32)
    left = np.zeros_like(raw)
    left[:, 3:] = raw[:, :-3]
    up = np.zeros_like(raw)
    up[1:] = raw[:-1]
    up_left = np.zeros_like(raw)
    up_left[1:, 3:] = raw[:-1, :-3]
    p = left + up - up_left
    pa, pb, pc = abs(p - left), abs(p - up), abs(p - up_left)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, up_left))
    predictions = np.stack([np.zeros_like(raw), left, up, (left + up) >> 1, paeth])
    residuals = ((raw[None] - predictions) & 255).astype(np.uint8)
    costs = np.abs(residuals.view(np.int8).astype(np.int64)).sum(axis=2)
    best = np.argmin(costs, axis=0)
    out = np.empty((height, 1 + 3 * width), np.uint8)
    out[:, 0] = best
    out[:, 1:] = residuals[best, np.arange(height)]
    return out


# ---- tokens ---------------------------------------------------------------------------------------------------------

def match_lengths(flat, distance, unit_end):
    """At every position the number of consecutive j >= i inside the unit with j - d >= 0 and F[j] = F[j - d], capped"""
    count = len(flat)
    equal = np.zeros(count, bool)
    if distance < count:
        equal[distance:] = flat[distance:] == flat[:-distance]
    index = np.arange(count, dtype=np.int64)
    stop = np.where(equal, count, index)
    stop = np.minimum.accumulate(stop[::-1])[::-1]
    return np.minimum(np.minimum(stop, unit_end) - index, MAX_MATCH)


def parse(stream):
    """The tokens of the rule for F (rows, row_length): (positions, lengths, distances) in stream order; length 1 and
    distance 0 for a literal"""
    rows, row_length = stream.shape
    flat = stream.reshape(-1)
    count = len(flat)
    index = np.arange(count, dtype=np.int64)
    in_row = index % row_length
    unit_end = index - in_row + np.minimum((in_row // UNIT + 1) * UNIT, row_length)
    candidates = [1, 3] + ([row_length] if row_length <= 32768 else [])
    best = np.zeros(count, np.int64)
    best_distance = np.zeros(count, np.int64)
    for distance in candidates:
        length = match_lengths(flat, distance, unit_end)
        better = length > best
        best[better] = length[better]
        best_distance[better] = distance
    step = np.where(best >= 3, best, 1)
    # the greedy chain from every unit's start
    start = np.zeros(count, bool)
    unit_starts = index[(in_row % UNIT) == 0]
    step_list = step.tolist()
    ends = unit_end[unit_starts].tolist()
    for first, end in zip(unit_starts.tolist(), ends):
        i = first
        while i < end:
            start[i] = True
            i += step_list[i]
    positions = index[start]
    lengths = step[start]
    distances = np.where(lengths >= 3, best_distance[start], 0)
    return positions, lengths, distances


# ---- codes ----------------------------------------------------------------------------------------------------------

def huffman_lengths(counts, limit):
    """CODES of the rule.  Returns (lengths, halvings)."""
    counts = [int(c) for c in counts]
    # so that the set of codes is complete: the lowest symbols without a count get one until two symbols have one
    for symbol in range(len(counts)):
        if sum(1 for c in counts if c) >= 2:
            break
        if counts[symbol] == 0:
            counts[symbol] = 1
    halvings = 0
    while True:
        leaves = sorted((c, s) for s, c in enumerate(counts) if c)
        m = len(leaves)
        weights, leaf_parent, node_parent = [], [0] * m, [0] * (m - 1)
        i = h = 0
        for k in range(m - 1):
            total = 0
            for _ in range(2):
                # the lighter of the next leaf and the next internal node; the leaf if they weigh the same
                if i < m and (h >= k or leaves[i][0] <= weights[h]):
                    total += leaves[i][0]
                    leaf_parent[i] = k
                    i += 1
                else:
                    total += weights[h]
                    node_parent[h] = k
                    h += 1
            weights.append(total)
        depth = [0] * (m - 1)
        for k in range(m - 3, -1, -1):
            depth[k] = depth[node_parent[k]] + 1
        lengths = [0] * len(counts)
        for i, (_, symbol) in enumerate(leaves):
            lengths[symbol] = depth[leaf_parent[i]] + 1
        if max(lengths) <= limit:
            return np.array(lengths), halvings
        counts = [(c + 1) >> 1 if c else 0 for c in counts]
        halvings += 1


def canonical_codes(lengths):
    """RFC 1951 3.2.2; returned with their bits reversed, as they go into the stream (least significant bit first)"""
    lengths = [int(n) for n in lengths]
    next_code, code = {}, 0
    for bits in range(1, 16):
        code = (code + sum(1 for n in lengths if n == bits - 1 and n)) << 1
        next_code[bits] = code
    out = []
    for n in lengths:
        if n == 0:
            out.append(0)
            continue
        value = next_code[n]
        next_code[n] += 1
        out.append(int(format(value, "0%db" % n)[::-1], 2))
    return np.array(out, np.int64)


def length_symbols(lengths):
    index = np.searchsorted(LENGTH_BASE, lengths, side="right") - 1
    return index, lengths - LENGTH_BASE[index]


def distance_symbols(distances):
    index = np.searchsorted(DISTANCE_BASE, distances, side="right") - 1
    return index, distances - DISTANCE_BASE[index]


def pack_bits(values, widths):
    """The fields, each least significant bit first, one behind the other: (bytes, with a zero-padded last byte; bits)"""
    values, widths = np.asarray(values, np.int64), np.asarray(widths, np.int64)
    total = int(widths.sum())
    if total == 0:
        return b"", 0
    field = np.repeat(np.arange(len(widths)), widths)
    within = np.arange(total) - np.repeat(np.cumsum(widths) - widths, widths)
    bits = ((values[field] >> within) & 1).astype(np.uint8)
    return np.packbits(bits, bitorder="little").tobytes(), total


def code_segment(flat, positions, lengths, distances, last):
    """One deflate block for the tokens of a segment.  Returns (its fields as (values, widths), statistics)."""
    literal = lengths < 3
    length_index, length_rest = length_symbols(lengths[~literal])
    distance_index, distance_rest = distance_symbols(distances[~literal])
    symbols = np.empty(len(positions), np.int64)
    symbols[literal] = flat[positions[literal]]
    symbols[~literal] = 257 + length_index
    literal_counts = np.bincount(symbols, minlength=LITERAL_COUNT)
    literal_counts[256] += 1
    distance_counts = np.bincount(distance_index, minlength=DISTANCE_COUNT)
    literal_extra = np.concatenate([np.zeros(257, np.int64), LENGTH_EXTRA])
    literal_lengths, literal_halvings = huffman_lengths(literal_counts, 15)
    distance_lengths, _ = huffman_lengths(distance_counts, 15)
    all_lengths = np.concatenate([literal_lengths, distance_lengths])
    meta_lengths, meta_halvings = huffman_lengths(np.bincount(all_lengths, minlength=19), 7)
    dynamic_bits = 14 + 57 + int(meta_lengths[all_lengths].sum()) + int((literal_counts * (literal_lengths + literal_extra)).sum()) + int((distance_counts * (distance_lengths + DISTANCE_EXTRA)).sum())
    fixed_bits = int((literal_counts * (FIXED_LITERAL_LENGTHS[:LITERAL_COUNT] + literal_extra)).sum()) + int((distance_counts * (FIXED_DISTANCE_LENGTHS + DISTANCE_EXTRA)).sum())
    dynamic = dynamic_bits < fixed_bits
    values, widths = [1 if last else 0, 2 if dynamic else 1], [1, 2]
    if dynamic:
        meta_codes = canonical_codes(meta_lengths)
        values += [29, 29, 15] + [int(meta_lengths[s]) for s in CODE_LENGTH_ORDER]
        widths += [5, 5, 4] + [3] * 19
        values += meta_codes[all_lengths].tolist()
        widths += meta_lengths[all_lengths].tolist()
    else:
        literal_lengths, distance_lengths = FIXED_LITERAL_LENGTHS, FIXED_DISTANCE_LENGTHS
    literal_codes, distance_codes = canonical_codes(literal_lengths), canonical_codes(distance_lengths)
    # per token up to four fields: the literal or length symbol, the rest of the length, the distance symbol, its rest
    token_values = np.zeros((len(positions), 4), np.int64)
    token_widths = np.zeros((len(positions), 4), np.int64)
    token_values[:, 0] = literal_codes[symbols]
    token_widths[:, 0] = literal_lengths[symbols]
    token_values[~literal, 1] = length_rest
    token_widths[~literal, 1] = LENGTH_EXTRA[length_index]
    token_values[~literal, 2] = distance_codes[distance_index]
    token_widths[~literal, 2] = distance_lengths[distance_index]
    token_values[~literal, 3] = distance_rest
    token_widths[~literal, 3] = DISTANCE_EXTRA[distance_index]
    values = np.concatenate([np.array(values, np.int64), token_values.reshape(-1), [literal_codes[256]]])
    widths = np.concatenate([np.array(widths, np.int64), token_widths.reshape(-1), [literal_lengths[256]]])
    statistics = {"dynamic": bool(dynamic), "literal_halvings": literal_halvings, "meta_halvings": meta_halvings, "tokens": len(positions),
                  "matches": int((~literal).sum()), "distance_symbols": int((distance_counts > 0).sum()),
                  "dynamic_bits": 3 + dynamic_bits, "fixed_bits": 3 + fixed_bits}
    return values, widths, statistics


def encode_stream(stream, width=None, height=None):
    """The file for a filtered stream F (rows, row_length) of bytes.  width, height: what IHDR says (default: row_length
    and rows, as the probe of include/vkr_png.h does).  Returns (bytes, a list of statistics per segment)."""
    stream = np.ascontiguousarray(stream, np.uint8)
    rows, row_length = stream.shape
    flat = stream.reshape(-1)
    positions, lengths, distances = parse(stream)
    per_segment = rows_per_segment(row_length, rows)
    segments = (rows + per_segment - 1) // per_segment
    pieces = [header(row_length if width is None else width, rows if height is None else height)]
    statistics = []
    borders = np.searchsorted(positions, np.arange(segments + 1) * per_segment * row_length)
    for n in range(segments):
        chosen = slice(borders[n], borders[n + 1])
        last = n == segments - 1
        values, widths, segment_statistics = code_segment(flat, positions[chosen], lengths[chosen], distances[chosen], last)
        if not last:
            # an empty stored block: 000, zeros to the byte border, then LEN and NLEN
            values, widths = np.concatenate([values, [0]]), np.concatenate([widths, [3]])
        data, _ = pack_bits(values, widths)
        data = (b"\x78\x5e" if n == 0 else b"") + data + (struct.pack(">I", zlib.adler32(flat.tobytes()) & 0xFFFFFFFF) if last else b"\x00\x00\xff\xff")
        pieces.append(chunk(b"IDAT", data))
        segment_statistics["bytes"] = len(data)
        statistics.append(segment_statistics)
    pieces.append(chunk(b"IEND", b""))
    return b"".join(pieces), statistics


def encode(image, statistics=False):
    """The bytes of the file of a uint8 image (height, width, 3 or 4; a fourth channel is ignored)"""
    stream = filtered_stream(image)
    if not valid_extent(image.shape[1], image.shape[0]):
        raise ValueError("a PNG file of the encoder is between 1 x 1 and 65535 x 65535 pixels")
    data, per_segment = encode_stream(stream, image.shape[1], image.shape[0])
    return (data, per_segment) if statistics else data


# ---- reading --------------------------------------------------------------------------------------------------------

def chunks(data):
    """[(kind, bytes)] of a file; every CRC is checked"""
    if data[:8] != SIGNATURE:
        raise ValueError("not a PNG file")
    at, out = 8, []
    while at < len(data):
        size, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + size]
        if len(body) != size or struct.unpack(">I", data[at + 8 + size:at + 12 + size])[0] != (zlib.crc32(kind + body) & 0xFFFFFFFF):
            raise ValueError("chunk %r at %d is cut off or fails its CRC" % (kind, at))
        out.append((kind, body))
        at += 12 + size
    if not out or out[0][0] != b"IHDR" or out[-1][0] != b"IEND" or out[-1][1]:
        raise ValueError("a PNG file begins with IHDR and ends with an empty IEND")
    return out


def inflated(data):
    """The inflated concatenation of the IDAT chunks of a file: the filtered stream (zlib checks the Adler-32)"""
    return zlib.decompress(b"".join(body for kind, body in chunks(data) if kind == b"IDAT"))


def decode(data):
    """The image (height, width, 3) of an 8-bit RGB file without interlacing"""
    width, height, bits, colour, compression, filtering, interlace = struct.unpack(">IIBBBBB", chunks(data)[0][1])
    if (bits, colour, compression, filtering, interlace) != (8, 2, 0, 0, 0):
        raise ValueError("only 8-bit RGB without interlacing is read")
    stream = np.frombuffer(inflated(data), np.uint8)
    if len(stream) != height * (3 * width + 1):
        raise ValueError("%d bytes of filtered stream instead of %d" % (len(stream), height * (3 * width + 1)))
    stream = stream.reshape(height, 3 * width + 1)
    out = np.zeros((height, 3 * width), np.uint8)
    above = np.zeros(3 * width, np.int32)
    for y in range(height):
        kind, residual = int(stream[y, 0]), stream[y, 1:].astype(np.int32)
        if kind == 0:
            row = residual
        elif kind == 2:
            row = (residual + above) & 255
        elif kind == 1:
            # three interleaved running sums
            row = np.zeros(3 * width, np.int32)
            for c in range(3):
                row[c::3] = np.cumsum(residual[c::3]) & 255
        elif kind in (3, 4):
            row = np.zeros(3 * width, np.int32)
            values, up = residual.tolist(), above.tolist()
            line = [0] * (3 * width)
            for x in range(3 * width):
                a = line[x - 3] if x >= 3 else 0
                b = up[x]
                if kind == 3:
                    predicted = (a + b) >> 1
                else:
                    c = up[x - 3] if x >= 3 else 0
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    predicted = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                line[x] = (values[x] + predicted) & 255
            row = np.array(line, np.int32)
        else:
            raise ValueError("row %d has filter %d" % (y, kind))
        out[y] = row
        above = row
    return out.reshape(height, width, 3)


def main(argv):
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("input", help="*.npy (uint8, height x width x 3 or 4)")
    ap.add_argument("output", help="the *.png to write")
    args = ap.parse_args(argv)
    image = np.ascontiguousarray(np.load(args.input), np.uint8)
    from . import renderer
    r = renderer.Renderer()
    try:
        data = r.encode_png(image)
    finally:
        r.close()
    with open(args.output, "wb") as file:
        file.write(data)
    print("Wrote %s: %d x %d, %d bytes." % (args.output, image.shape[1], image.shape[0], len(data)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
