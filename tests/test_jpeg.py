"""JPEG files (include/vkr_jpeg.h) on the CPU: the numpy restatement vulkan_renderer_amd/jpeg.py against the files that
the reference's writer made (tests/golden/jpeg.npz, written by tests/golden/make_jpeg.py) and against the live writer
where oracle/_ref is present; that the fixtures reach every path of the entropy coder; the header and its tables; the
worst-case size; the host part of the library (tables, header, capacity, refusals, file writer)."""
import ctypes as C

import numpy as np
import pytest

import jpeg_cases
from vulkan_renderer_amd import capi, jpeg

FIXTURES = jpeg_cases.fixtures()
EXPECTED_FIXTURES = {"pixel_q70": (1, 1, 70), "noise_16x16_q70": (16, 16, 70), "ramp_17x9_q70": (17, 9, 70), "ramp_33x31_q70": (33, 31, 70),
                     "noise_136x72_q70": (136, 72, 70), "noise_40x24_q95": (40, 24, 95), "noise_40x24_q100": (40, 24, 100),
                     "checkerboard_32x32_q100": (32, 32, 100), "sparse_136x72_q70": (136, 72, 70), "white_24x24_q100": (24, 24, 100),
                     "noise_32x16_q1": (32, 16, 1), "stripes_32x32_q100": (32, 32, 100)}


def test_the_fixture_set_is_the_one_the_tests_rely_on():
    assert {name: (image.shape[1], image.shape[0], quality) for name, (image, quality, _) in FIXTURES.items()} == EXPECTED_FIXTURES
    checkerboard = FIXTURES["checkerboard_32x32_q100"][0]
    assert set(np.unique(checkerboard)) == {0, 255} and (checkerboard[:8, :8] == checkerboard[0, 0]).all() and checkerboard[0, 8, 0] != checkerboard[0, 0, 0]
    assert (FIXTURES["white_24x24_q100"][0] == 255).all()
    stripes = FIXTURES["stripes_32x32_q100"][0]
    assert (stripes[0, 0::2] == 0).all() and (stripes[0, 1::2] == 255).all()


@pytest.mark.parametrize("name", sorted(EXPECTED_FIXTURES))
def test_restatement_equals_the_writers_file(name):
    image, quality, expected = FIXTURES[name]
    got, statistics = jpeg.encode(image, quality)
    print(name, len(got), {k: v for k, v in statistics.items() if k != "stuffed_positions"})
    assert jpeg_cases.first_difference(got, expected) is None
    # RGBA input: alpha is ignored
    rgba = np.concatenate([image, np.full(image.shape[:2] + (1,), 77, np.uint8)], axis=-1)
    assert jpeg.encode(rgba, quality)[0] == expected


def test_fixtures_reach_every_path_of_the_entropy_coder():
    statistics = {name: jpeg.encode(image, quality)[1] for name, (image, quality, _) in FIXTURES.items()}
    total = {key: sum(int(s[key]) for s in statistics.values()) for key in
             ("zrl_codes", "double_zrl", "data_units_without_eob", "data_units_all_ac_zero", "zero_dc_differences", "stuffed_bytes", "last_byte_stuffed", "ends_aligned")}
    largest_ac = max(s["largest_ac_category"] for s in statistics.values())
    print(total, "largest AC category reached:", largest_ac)
    for key in ("zrl_codes", "double_zrl", "data_units_without_eob", "data_units_all_ac_zero", "zero_dc_differences", "stuffed_bytes"):
        assert total[key] > 0, key
    assert total["last_byte_stuffed"] + total["ends_aligned"] > 0
    assert max(s["largest_dc_category"] for s in statistics.values()) == 11
    # what the table of the fixtures claims of single ones
    assert statistics["sparse_136x72_q70"]["double_zrl"] > 0
    assert statistics["noise_136x72_q70"]["data_units"] == 270
    big = statistics["noise_136x72_q70"]
    assert min(big["zrl_codes"], big["data_units_without_eob"], big["stuffed_bytes"], big["zero_dc_differences"], big["data_units_all_ac_zero"]) > 0
    assert statistics["noise_40x24_q100"]["data_units_without_eob"] == statistics["noise_40x24_q100"]["data_units"] == 45
    # chroma is subsampled up to quality 90: the writer's file at 95 has 8 x 8 MCUs of three data units, like the one at 100
    assert statistics["noise_40x24_q95"]["data_units"] == 5 * 3 * 3 and FIXTURES["noise_40x24_q95"][2][0x9A + 11] == 0x11
    assert statistics["noise_32x16_q1"]["data_units"] == 2 * 1 * 6 and FIXTURES["noise_32x16_q1"][2][0x9A + 11] == 0x22
    assert statistics["checkerboard_32x32_q100"]["largest_dc_category"] == 11
    assert statistics["checkerboard_32x32_q100"]["data_units_all_ac_zero"] == 48 and statistics["checkerboard_32x32_q100"]["stuffed_bytes"] > 0
    assert largest_ac == statistics["stripes_32x32_q100"]["largest_ac_category"]
    # quality 1: every table entry above 255 / 50 is clamped
    assert (jpeg.quantisation_tables(1)[0] == 255).sum() > 32


@pytest.mark.skipif(not jpeg_cases.reference_available(), reason="oracle/_ref is not built")
def test_restatement_equals_the_live_writer_on_random_extents():
    rng = np.random.default_rng(2024)
    for _ in range(50):
        width, height = int(rng.integers(1, 81)), int(rng.integers(1, 81))
        quality = int(rng.choice([0, 1, 5, 30, 49, 50, 70, 89, 90, 91, 95, 100, int(rng.integers(1, 101))]))
        channels = int(rng.integers(3, 5))
        kind = int(rng.integers(0, 3))
        image = rng.integers(0, 256, (height, width, channels), dtype=np.uint8)
        if kind == 1:  # smooth: long runs of zeros
            image = (image // 32 + np.linspace(0, 200, width)[None, :, None]).astype(np.uint8)
        elif kind == 2:  # two levels: large coefficients
            image = ((image > 127) * 255).astype(np.uint8)
        assert jpeg_cases.first_difference(jpeg.encode(image, quality)[0], jpeg_cases.reference_file(image, quality)) is None, (width, height, quality, channels, kind)


def segments(header):
    """marker -> payload of the segments of a header"""
    assert header[:2] == b"\xFF\xD8"
    at, out = 2, {}
    while at < len(header):
        assert header[at] == 0xFF
        length = int.from_bytes(header[at + 2:at + 4], "big")
        out[header[at + 1]] = header[at + 4:at + 2 + length]
        at += 2 + length
    assert at == len(header)
    return out


def test_header_holds_the_annex_k_tables():
    header = jpeg.header(40, 24, 50)
    assert len(header) == jpeg.HEADER_SIZE == capi.JPEG_HEADER_SIZE == 607
    for name, (image, quality, expected) in FIXTURES.items():
        assert jpeg.header(image.shape[1], image.shape[0], quality) == expected[:607], name
    parts = segments(header)
    assert sorted(parts) == [0xC0, 0xC4, 0xDA, 0xDB, 0xE0]
    assert parts[0xE0] == b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0"
    # quality 50 scales by 100 / 100: the entries are the base tables, in zig-zag order
    dqt = parts[0xDB]
    assert len(dqt) == 130 and dqt[0] == 0 and dqt[65] == 1
    assert np.array_equal(np.frombuffer(dqt[1:65], np.uint8)[jpeg.ZIGZAG], jpeg.K1)
    assert np.array_equal(np.frombuffer(dqt[66:130], np.uint8)[jpeg.ZIGZAG], jpeg.K2)
    assert list(jpeg.ZIGZAG[:10]) == [0, 1, 5, 6, 14, 15, 27, 28, 2, 4] and sorted(jpeg.ZIGZAG) == list(range(64))
    assert parts[0xC0] == bytes([8, 0, 24, 0, 40, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    assert segments(jpeg.header(40, 24, 91))[0xC0][7] == 0x11
    assert parts[0xDA] == bytes([3, 1, 0, 2, 0x11, 3, 0x11, 0, 63, 0])
    dht, at = parts[0xC4], 0
    for class_and_id, (counts, symbols) in zip(jpeg.HUFFMAN_CLASS_AND_ID, jpeg.HUFFMAN_SPECIFICATIONS):
        assert dht[at] == class_and_id and list(dht[at + 1:at + 17]) == counts and list(dht[at + 17:at + 17 + sum(counts)]) == symbols
        assert len(set(symbols)) == len(symbols) == sum(counts)
        at += 17 + sum(counts)
    assert at == len(dht)
    assert len(jpeg.AC_LUMINANCE[1]) == len(jpeg.AC_CHROMINANCE[1]) == 162


def test_derived_code_words_are_prefix_free():
    for specification in jpeg.HUFFMAN_SPECIFICATIONS:
        codes = jpeg.huffman_codes(specification)
        words = sorted(format(int(code), "0%db" % length) for code, length in codes if length)
        assert len(words) == len(specification[1])
        for shorter, longer in zip(words, words[1:]):
            assert not longer.startswith(shorter)
        assert all(set(word) != {"1"} for word in words)  # T.81 C.2: no code of ones only
    # two code words of each kind as Annex K prints them
    assert tuple(jpeg.huffman_codes(jpeg.DC_LUMINANCE)[0]) == (0, 2) and tuple(jpeg.huffman_codes(jpeg.DC_CHROMINANCE)[11]) == (0x7FE, 11)
    assert tuple(jpeg.huffman_codes(jpeg.AC_LUMINANCE)[0x00]) == (0b1010, 4) and tuple(jpeg.huffman_codes(jpeg.AC_LUMINANCE)[0xF0]) == (0x7F9, 11)
    assert tuple(jpeg.huffman_codes(jpeg.AC_CHROMINANCE)[0x00]) == (0, 2) and tuple(jpeg.huffman_codes(jpeg.AC_CHROMINANCE)[0xF0]) == (0x3FA, 10)


def test_capacity_bounds_every_file():
    lib = capi.load()
    for name, (image, quality, expected) in FIXTURES.items():
        bound = lib.get_jpeg_capacity(image.shape[1], image.shape[0], quality)
        assert bound == jpeg.capacity(image.shape[1], image.shape[0], quality), name
        assert bound >= len(expected), name
    # 22 bits of DC and 63 times 26 bits of AC per data unit
    assert jpeg.capacity(8, 8, 100) == 607 + 2 * ((3 * (22 + 63 * 26) + 7) // 8 + 1) + 2
    # adversarial inputs at quality 100: 1-pixel stripes, 1-pixel checkerboard, two-level noise
    y, x = np.mgrid[0:48, 0:64]
    rng = np.random.default_rng(5)
    for image in (FIXTURES["stripes_32x32_q100"][0], np.repeat((((x + y) % 2) * 255).astype(np.uint8)[..., None], 3, axis=-1),
                  (rng.integers(0, 2, (48, 64, 3)) * 255).astype(np.uint8), (rng.integers(0, 2, (48, 64, 1)) * 255).astype(np.uint8).repeat(3, axis=-1)):
        size = len(jpeg.encode(image, 100)[0])
        bound = lib.get_jpeg_capacity(image.shape[1], image.shape[0], 100)
        print(image.shape, size, bound)
        assert size < bound
    assert lib.get_jpeg_capacity(0, 8, 70) == 0 and lib.get_jpeg_capacity(8, 65536, 70) == 0
    assert lib.get_jpeg_capacity(65535, 1, 70) > 0


def test_library_header_equals_the_restatement():
    lib = capi.load()
    for width, height, quality in ((1, 1, 70), (1920, 1080, 70), (65535, 3, 0), (40, 24, 90), (40, 24, 91), (7, 300, 1), (8, 8, 100), (5, 5, -3), (5, 5, 1000), (9, 9, 25), (9, 9, 50)):
        header = (C.c_uint8 * 607)()
        assert lib.get_jpeg_header(header, width, height, quality) == 0
        assert bytes(header) == jpeg.header(width, height, quality), (width, height, quality)
    assert lib.get_jpeg_header((C.c_uint8 * 607)(), 0, 5, 70) == 1 and lib.get_jpeg_header((C.c_uint8 * 607)(), 5, 65536, 70) == 1
    assert lib.get_jpeg_stuffing_chunk_size() == 64


def test_encoder_refuses_without_a_device_and_bad_extents():
    lib = capi.load()
    encoder = capi.JpegEncoder()
    for device, width, height, slots in ((None, 16, 16, 1),):
        encoder.width = 5
        assert lib.create_jpeg_encoder(C.byref(encoder), device, width, height, 70, slots) == 1
        assert bytes(encoder) == bytes(C.sizeof(encoder))
    lib.destroy_jpeg_encoder(C.byref(encoder))  # a zeroed encoder is destroyed without harm


def test_write_jpeg_writes_the_bytes(tmp_path):
    lib = capi.load()
    data = FIXTURES["ramp_17x9_q70"][2]
    path = str(tmp_path / "out.jpg")
    assert lib.write_jpeg(path.encode(), data, len(data)) == 0
    assert open(path, "rb").read() == data
    assert lib.write_jpeg(str(tmp_path / "missing" / "out.jpg").encode(), data, len(data)) == 1
