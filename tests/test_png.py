"""The rule of include/vkr_png.h without a GPU: the numpy restatement vulkan_renderer_amd/png.py against the files the
reference's writer made (tests/golden/png.npz) - it decodes to their images, its inflated IDAT stream is theirs byte for
byte and that of write_png_rgb8(), and over the golden frames its files are smaller -, against that writer itself where
oracle/_ref is present; tokens, codes, framing, capacity, header, rejected extents and the command line."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

import png_cases
from vulkan_renderer_amd import capi, png

FIXTURES = sorted(png_cases.fixtures())
GENERATED = sorted(png_cases.generated_cases())


def image_of(name):
    return png_cases.fixtures()[name][0] if name in png_cases.fixtures() else png_cases.generated_cases()[name]


def test_the_fixtures_are_the_golden_frames_and_the_generated_images():
    fixtures = png_cases.fixtures()
    with np.load(png_cases.FRAMES) as frames:
        assert png_cases.golden_frame_names() == sorted(frames.files) and len(frames.files) == 30
    import oracle
    for name, image in {**png_cases.golden_frame_images(), **png_cases.generated_fixture_images()}.items():
        assert np.array_equal(fixtures[name][0], image), name
    assert len(fixtures) == 35 and oracle.encode_srgb8(np.ones((1, 1, 4), np.float32))[0, 0, 0] == 255
    # what the device is held to covers all five filters
    assert set(png_cases.DEVICE_FIXTURES) <= set(fixtures)
    assert set(np.concatenate([png_cases.filters_of(fixtures[name][1]) for name in png_cases.DEVICE_FIXTURES]).tolist()) == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_decodes_to_the_image_with_the_writers_filtered_stream(name):
    image, reference_file = png_cases.fixtures()[name]
    data, statistics = png_cases.restated(name)
    assert np.array_equal(png_cases.decode(data), image) and np.array_equal(png.decode(data), image)
    width, height, stream = png_cases.inflated_idat(data)
    assert (width, height) == (image.shape[1], image.shape[0])
    assert stream == png_cases.inflated_idat(reference_file)[2] == png.filtered_stream(image).tobytes()
    assert len(data) <= png.capacity(width, height)
    assert len(png_cases.idat_sizes(data)) == len(statistics) == 1


@pytest.mark.parametrize("name", GENERATED)
def test_generated_cases_decode_and_stay_within_the_capacity(name):
    image = png_cases.generated_cases()[name]
    data, statistics = png_cases.restated(name)
    assert np.array_equal(png_cases.decode(data), image)
    assert png_cases.inflated_idat(data)[2] == png.filtered_stream(image).tobytes()
    assert len(data) <= png.capacity(image.shape[1], image.shape[0])
    assert png.decode(png.encode(np.concatenate([image, np.full(image.shape[:2] + (1,), 9, np.uint8)], axis=-1))).tobytes() == image.tobytes()
    if png_cases.reference_available():
        assert png_cases.inflated_idat(data)[2] == png_cases.inflated_idat(png_cases.reference_file(image))[2]


def test_what_the_generated_cases_are_there_for():
    statistics = {name: png_cases.restated(name)[1] for name in GENERATED}
    # two segments and two IDATs; a unit of three bytes
    assert len(statistics["render_like_1366x17"]) == 2 and png.rows_per_segment(4099, 17) == 15 and 4099 % png.UNIT == 3
    assert len(png_cases.idat_sizes(png_cases.restated("render_like_1366x17")[0])) == 2
    # the row distance is a candidate at 32767 and none at 32770
    assert 3 * 10922 + 1 == 32767 and 3 * 10923 + 1 == 32770
    assert statistics["few_values_10922x2"][0]["distance_symbols"] == 3 and max(s["distance_symbols"] for s in statistics["few_values_10923x2"]) == 2
    assert len(statistics["few_values_10922x2"]) == 1 and len(statistics["few_values_10923x2"]) == 2
    # the block choice
    assert statistics["noise_200x40"][0]["dynamic"] and not statistics["noise_2x2"][0]["dynamic"] and not statistics["pixel_1x1"][0]["dynamic"]
    # the cap: 901 equal bytes of a row are 258 + 258 + 258 + 126 behind one literal
    positions, lengths, distances = png.parse(png.filtered_stream(png_cases.generated_cases()["flat_300x9"]))
    assert lengths.max() == 258 and (lengths[lengths >= 3] <= 258).all() and set(distances.tolist()) <= {0, 1, 3, 901}
    # all filters tie on an all-zero image: filter 0
    assert (png.filtered_stream(png_cases.generated_cases()["zero_7x5"]) == 0).all()


def test_golden_frames_are_smaller_than_the_writers_files():
    """The condition of the design: dynamic codes and three distances beat the writer's fixed code and hash chains"""
    names = png_cases.golden_frame_names()
    ours = {name: len(png_cases.restated(name)[0]) for name in names}
    theirs = {name: len(png_cases.fixtures()[name][1]) for name in names}
    print("restatement %d bytes, reference writer %d bytes, ratio %.3f; larger: %s" % (sum(ours.values()), sum(theirs.values()), sum(ours.values()) / sum(theirs.values()),
                                                                                      [name for name in names if ours[name] > theirs[name]]))
    assert sum(ours.values()) < sum(theirs.values())


@pytest.mark.skipif(not png_cases.reference_available(), reason="oracle/_ref is not built")
def test_filtered_stream_equals_the_live_writer():
    rng = np.random.default_rng(30)
    for n in range(40):
        width, height = int(rng.integers(1, 90)), int(rng.integers(1, 12))
        kind = n % 4
        image = png_cases.noise(width, height, n) if kind == 0 else png_cases.render_like(width, height, n) if kind == 1 else png_cases.ramp(width, height) if kind == 2 else (png_cases.noise(width, height, n) // 64 * 64)
        assert png.filtered_stream(image).tobytes() == png_cases.inflated_idat(png_cases.reference_file(image))[2], (width, height, kind)


@pytest.mark.parametrize("name", FIXTURES + GENERATED)
def test_filtered_stream_is_that_of_write_png_rgb8(tmp_path, name):
    lib = capi.load()
    path = str(tmp_path / "host.png")
    image = np.ascontiguousarray(image_of(name))
    assert lib.write_png_rgb8(path.encode(), image.shape[1], image.shape[0], image.ctypes.data) == 0
    with open(path, "rb") as file:
        host = file.read()
    width, height, stream = png_cases.inflated_idat(host)
    assert (width, height) == (image.shape[1], image.shape[0])
    assert stream == png_cases.inflated_idat(png_cases.restated(name)[0])[2]
    assert np.array_equal(png_cases.unfilter(stream, width, height), image)


# ---- tokens and codes -------------------------------------------------------------------------------------------------

def greedy_tokens(stream):
    """TOKENS of the rule, position by position"""
    rows, row_length = stream.shape
    flat = stream.reshape(-1).tolist()
    distances = [1, 3] + ([row_length] if row_length <= 32768 else [])
    out = []
    for row in range(rows):
        for first in range(0, row_length, png.UNIT):
            i, end = row * row_length + first, row * row_length + min(first + png.UNIT, row_length)
            while i < end:
                best, best_distance = 0, 0
                for d in distances:
                    n = 0
                    while i + n < end and n < 258 and i + n - d >= 0 and flat[i + n] == flat[i + n - d]:
                        n += 1
                    if n > best:
                        best, best_distance = n, d
                if best >= 3:
                    out.append((i, best, best_distance))
                    i += best
                else:
                    out.append((i, 1, 0))
                    i += 1
    return out


def test_the_vectorised_parse_is_the_greedy_walk():
    rng = np.random.default_rng(31)
    for rows, row_length, values in ((3, 10, 2), (4, 7, 3), (2, 4100, 2), (1, 1, 5), (6, 3, 2), (3, 600, 1), (2, 5000, 4), (5, 1, 2)):
        stream = rng.integers(0, values, (rows, row_length), dtype=np.uint8)
        positions, lengths, distances = png.parse(stream)
        assert list(zip(positions.tolist(), lengths.tolist(), distances.tolist())) == greedy_tokens(stream), (rows, row_length)


def kraft(lengths):
    return sum(2.0 ** -int(n) for n in lengths if n)


def test_code_lengths_are_complete_limited_and_deterministic():
    rng = np.random.default_rng(32)
    for n in range(200):
        size = int(rng.choice([19, 30, 286]))
        counts = (rng.integers(0, 1000, size) * (rng.random(size) < rng.random())).astype(np.int64)
        limit = 7 if size == 19 else 15
        lengths, _ = png.huffman_lengths(counts, limit)
        assert kraft(lengths) == 1.0 and lengths.max() <= limit
        # every symbol with a count has a code, and a rarer symbol never a shorter one
        used = np.nonzero(counts)[0]
        assert (lengths[used] > 0).all()
        order = used[np.argsort(counts[used], kind="stable")]
        assert (np.diff(lengths[order]) <= 0).all()
    # the padding: no count, one count
    assert png.huffman_lengths([0] * 30, 15)[0].tolist() == [1, 1] + [0] * 28
    assert png.huffman_lengths([0, 0, 7] + [0] * 27, 15)[0].tolist() == [1, 0, 1] + [0] * 27
    # Fibonacci counts: 1, 1, 2, 3, ... make a chain; 17 of them give 16 bits and are halved until 15 are enough
    fibonacci = [1, 1]
    while len(fibonacci) < 17:
        fibonacci.append(fibonacci[-1] + fibonacci[-2])
    lengths, halvings = png.huffman_lengths(fibonacci, 15)
    assert halvings >= 1 and lengths.max() <= 15 and kraft(lengths) == 1.0
    lengths, halvings = png.huffman_lengths(fibonacci[:16], 15)
    assert lengths.tolist() == [15, 15] + list(range(14, 0, -1)) and halvings == 0
    # ties: equal counts are joined in the order of their symbols, a leaf before a joined node of the same weight
    assert png.huffman_lengths([1, 1, 1, 1], 15)[0].tolist() == [2, 2, 2, 2]
    assert png.huffman_lengths([1, 1, 2], 15)[0].tolist() == [2, 2, 1]
    assert png.huffman_lengths([2, 1, 1, 2], 15)[0].tolist() == [2, 2, 2, 2]
    # canonical codes of RFC 1951 3.2.2, its example: lengths 3, 3, 3, 3, 3, 2, 4, 4
    codes = png.canonical_codes([3, 3, 3, 3, 3, 2, 4, 4])
    assert [format(int(c), "0%db" % n)[::-1] for c, n in zip(codes, [3, 3, 3, 3, 3, 2, 4, 4])] == ["010", "011", "100", "101", "110", "00", "1110", "1111"]


@pytest.mark.parametrize("name", sorted(png_cases.probe_streams()))
def test_probe_streams_inflate_to_themselves(name):
    stream = png_cases.probe_streams()[name]
    data, statistics = png_cases.restated_stream(name)
    chunks = png_cases.read_chunks(data)
    assert struct.unpack(">II", chunks[0][1][:8]) == (stream.shape[1], stream.shape[0])
    assert zlib.decompress(b"".join(body for kind, body in chunks if kind == b"IDAT")) == stream.tobytes()
    assert len(data) <= png.stream_capacity(stream.shape[1], stream.shape[0])
    assert len(statistics) == len(chunks) - 2


def test_what_the_probe_streams_are_there_for():
    statistics = {name: png_cases.restated_stream(name)[1] for name in png_cases.probe_streams()}
    assert all(s["literal_halvings"] >= 1 and s["matches"] == 0 and s["dynamic"] for s in statistics["fibonacci"])
    assert statistics["meta_code"][0]["meta_halvings"] >= 1 and statistics["meta_code"][0]["dynamic"] and statistics["meta_code"][0]["matches"] == 0
    assert len(statistics["all_ff_70000"]) == 2 and png_cases.probe_streams()["all_ff_70000"].size == 70000
    assert statistics["single_value"][0]["distance_symbols"] == 1 and statistics["one_distance"][0]["distance_symbols"] == 1
    assert set(png.parse(png_cases.probe_streams()["one_distance"])[2].tolist()) == {0, 3}
    assert len(statistics["long_rows"]) == 2 and len(statistics["noise_rows_of_one"]) == 1


# ---- framing, header, capacity ----------------------------------------------------------------------------------------

def test_framing():
    data, statistics = png_cases.restated("render_like_1366x17")
    chunks = png_cases.read_chunks(data)
    assert [kind for kind, _ in chunks] == [b"IHDR", b"IDAT", b"IDAT", b"IEND"]
    first, second = chunks[1][1], chunks[2][1]
    assert first[:2] == b"\x78\x5e" and first[-4:] == b"\x00\x00\xff\xff"
    flat = png.filtered_stream(png_cases.generated_cases()["render_like_1366x17"]).tobytes()
    assert second[-4:] == struct.pack(">I", zlib.adler32(flat))
    # each IDAT ends at a block border: the first inflates on its own to the rows of its segment
    inflater = zlib.decompressobj()
    assert inflater.decompress(first) == flat[:15 * 4099] and not inflater.eof
    assert inflater.decompress(second) == flat[15 * 4099:] and inflater.eof
    # BFINAL and BTYPE: dynamic blocks, the last one final
    assert first[2] & 7 == 0b100 and second[0] & 7 == 0b101
    fixed, _ = png_cases.restated("noise_2x2")
    assert png_cases.read_chunks(fixed)[1][1][2] & 7 == 0b011


def test_header_capacity_and_rejected_extents():
    lib = capi.load()
    buffer = C.create_string_buffer(capi.PNG_HEADER_SIZE)
    for width, height in ((1, 1), (7, 5), (1366, 17), (1920, 1080), (10922, 2), (10923, 2), (21845, 3), (21846, 3), (65535, 65535), (1, 65535), (65535, 1)):
        assert lib.get_png_header(buffer, width, height) == 0 and buffer.raw == png.header(width, height) and len(png.header(width, height)) == capi.PNG_HEADER_SIZE
        assert lib.get_png_capacity(width, height) == png.capacity(width, height) > 0, (width, height)
    assert png.header(3, 2) == b"\x89PNG\r\n\x1a\n\x00\x00\x00\rIHDR\x00\x00\x00\x03\x00\x00\x00\x02\x08\x02\x00\x00\x00" + struct.pack(">I", zlib.crc32(b"IHDR\x00\x00\x00\x03\x00\x00\x00\x02\x08\x02\x00\x00\x00"))
    for width, height in ((0, 1), (1, 0), (65536, 1), (1, 65536)):
        assert lib.get_png_header(buffer, width, height) == 1 and lib.get_png_capacity(width, height) == 0 and png.capacity(width, height) == 0
    # the derivation: per segment of n bytes (9 n + 20) / 8 + 16, and 47 bytes around them
    assert png.capacity(1, 1) == 47 + (9 * 4 + 20) // 8 + 16 == 70
    assert png.capacity(1366, 17) == 47 + (9 * 15 * 4099 + 20) // 8 + 16 + (9 * 2 * 4099 + 20) // 8 + 16
    assert png.capacity(65535, 65535) == 47 + 65535 * ((9 * 196606 + 20) // 8 + 16) > 1 << 33
    for rows, row_length in ((1, 1), (7, 10000), (50, 1), (2, 262144), (65535, 4)):
        assert lib.get_png_stream_capacity(row_length, rows) == png.stream_capacity(row_length, rows)
    assert lib.get_png_stream_capacity(262145, 1) == 0 and lib.get_png_stream_capacity(0, 1) == 0 and lib.get_png_stream_capacity(1, 65536) == 0
    # device == NULL is an error and leaves the encoder zeroed
    encoder = capi.PngEncoder()
    assert lib.create_png_encoder(C.byref(encoder), None, 5, 5, 1) == 1 and not encoder.state and encoder.width == 0
    # a fixed-code token never takes more than nine bits per byte it covers
    lengths = np.arange(3, 259)
    index, _ = png.length_symbols(lengths)
    worst = png.FIXED_LITERAL_LENGTHS[257 + index] + png.LENGTH_EXTRA[index] + 5 + 13
    assert (worst <= 9 * lengths).all() and png.FIXED_LITERAL_LENGTHS[:256].max() == 9


def test_encode_refuses_what_is_no_image():
    for image in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 2), np.uint8), np.zeros((0, 4, 3), np.uint8), np.zeros((4, 4, 3), np.float32)):
        with pytest.raises(ValueError):
            png.encode(image)
    data = png_cases.restated("generated_noise_24x16")[0]
    for broken in (data[:-1], data[:40] + bytes([data[40] ^ 1]) + data[41:], b"\0" + data[1:]):
        with pytest.raises((ValueError, zlib.error, struct.error)):
            png.decode(broken)


def test_write_png_file_and_the_command_line_without_a_device(tmp_path):
    """write_png_file() writes what it is given; the command line of the module needs the device and is run by
    tests/test_gpu_png.py - here its arguments are parsed"""
    lib = capi.load()
    data = png_cases.restated("generated_ramp_40x24")[0]
    path = str(tmp_path / "file.png")
    assert lib.write_png_file(path.encode(), data, len(data)) == 0
    with open(path, "rb") as file:
        assert file.read() == data
    assert lib.write_png_file(str(tmp_path / "missing" / "file.png").encode(), data, len(data)) == 1
    with pytest.raises(SystemExit):
        png.main(["only_one_argument.npy"])
