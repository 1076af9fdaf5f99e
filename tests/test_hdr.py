"""The rule of include/vkr_hdr.h without a GPU: the numpy restatement vulkan_renderer_amd/hdr.py against the files the
reference's writer made (tests/golden/hdr.npz) and against that writer itself where oracle/_ref is present; the
statement of the run-length coding without a cursor against a cursor loop; capacity, decoding, sanitising and the way
through the half."""
import numpy as np
import pytest

import hdr_cases
from vulkan_renderer_amd import capi, hdr

F = np.float32


def test_the_fixtures_are_the_cases():
    cases, fixtures = hdr_cases.cases(), hdr_cases.fixtures()
    assert sorted(cases) == sorted(fixtures)
    for name, (image, through_half) in cases.items():
        assert fixtures[name][1] == through_half and np.array_equal(fixtures[name][0].view(np.uint32), image.view(np.uint32)), name
    # what the cases are there for
    widths = {image.shape[1] for image, _ in cases.values()}
    assert set(hdr_cases.WIDTHS) <= widths and {image.shape[0] for image, _ in cases.values()} >= {1, 2, 3, 4}
    assert hdr_cases.SEGMENT % hdr_cases.CHUNK == 0 and max(widths) > hdr_cases.SEGMENT + hdr_cases.CHUNK


@pytest.mark.parametrize("name", sorted(hdr_cases.cases()))
def test_restatement_equals_the_writers_file(name):
    image, through_half, expected = hdr_cases.fixtures()[name]
    assert hdr_cases.first_difference(hdr.encode(image, through_half), expected) is None


def random_image(rng):
    width = int(rng.choice([1, 5, 7, 8, 9, 31, 64, 127, 128, 129, 255, 256, 300, 385, int(rng.integers(1, 400))]))
    height = int(rng.integers(1, 5))
    kind = int(rng.integers(0, 4))
    if kind == 0:
        return (rng.random((height, width, 3), F) * F(10.0 ** rng.integers(-35, 37))).astype(F)
    if kind == 1:
        return rng.choice(np.array([0.5, 0.25], F), (height, width, 3), p=[0.9, 0.1])
    if kind == 2:
        return np.repeat(rng.random((height, width // 5 + 1, 3), F), 5, axis=1)[:, :width]
    return rng.choice(np.array([1.0, 3.0, 1e-33, 65504.0, hdr.FLT_MAX], F), (height, width, 3), p=[0.6, 0.3, 0.04, 0.04, 0.02])


@pytest.mark.skipif(not hdr_cases.reference_available(), reason="oracle/_ref is not built")
def test_restatement_equals_the_live_writer():
    rng = np.random.default_rng(20)
    for _ in range(50):
        image = random_image(rng)
        through_half = bool(rng.integers(0, 2)) and float(image.max()) <= 65504.0
        assert hdr_cases.first_difference(hdr.encode(image, through_half), hdr_cases.reference_file(image, through_half)) is None, image.shape


@pytest.mark.parametrize("name", sorted(hdr_cases.cases()))
def test_decoding_gives_the_rgbe_bytes_back(name):
    image, through_half = hdr_cases.cases()[name]
    assert np.array_equal(hdr.decode(hdr.encode(image, through_half)), hdr.rgbe(image, through_half))


def test_decoding_refuses_what_is_cut_off():
    data = hdr.encode(hdr_cases.cases()["constant_300x2"][0])
    with pytest.raises((ValueError, IndexError)):
        hdr.decode(data[:-1])
    with pytest.raises(ValueError):
        hdr.decode(data + b"\0")


def test_capacity_is_never_exceeded_and_reached_without_runs():
    for name, (image, through_half) in hdr_cases.cases().items():
        assert len(hdr.encode(image, through_half)) <= hdr.capacity(image.shape[1], image.shape[0]), name
    image = hdr_cases.cases()["no_runs_256x1"][0]
    assert len(hdr.encode(image)) == hdr.capacity(256, 1) == len(hdr.header(256, 1)) + 4 + 4 * (256 + 2)
    # a plane of 129 bytes without a run has two packets
    assert hdr.code_planes(hdr_cases.background(129)[None])[1][0] == 129 + 2
    assert hdr.capacity(7, 3) == len(hdr.header(7, 3)) + 84 and hdr.capacity(32768, 1) == len(hdr.header(32768, 1)) + 4 * 32768
    assert hdr.capacity(0, 1) == 0 and hdr.capacity(1, 65536) == 0
    assert hdr.capacity(32767, 65535) == len(hdr.header(32767, 65535)) + 65535 * (4 + 4 * (32767 + 256)) > 1 << 33


def cursor_loop(plane):
    """The run-length coding with a cursor, as the format's writers state it: look for the next three equal bytes, dump
    what lies before them in packets of at most 128, then the run of equal bytes in packets of at most 127"""
    plane, out, x, width = list(plane), [], 0, len(plane)
    while x < width:
        r = x
        while r + 2 < width and not (plane[r] == plane[r + 1] == plane[r + 2]):
            r += 1
        if r + 2 >= width:
            r = width
        while x < r:
            n = min(128, r - x)
            out += [n] + plane[x:x + n]
            x += n
        if r + 2 < width:
            while r < width and plane[r] == plane[x]:
                r += 1
            while x < r:
                n = min(127, r - x)
                out += [128 + n, plane[x]]
                x += n
    return bytes(out)


def test_the_statement_without_a_cursor_equals_the_cursor_loop():
    rng = np.random.default_rng(21)
    widths = rng.choice([8, 9, 10, 11, 63, 64, 65, 126, 127, 128, 129, 130, 254, 255, 256, 257, 258, 300, 400], 10000)
    total = 0
    for alphabet in (2, 3):
        for width in sorted(set(widths)):
            count = int((widths == width).sum()) // 2 + 1
            # (half of them with long stretches: symbols repeated 1 ... 140 times)
            planes = rng.integers(0, alphabet, (count, width)).astype(np.uint8)
            for row in planes[::2]:
                row[:] = np.repeat(rng.integers(0, alphabet, width), rng.integers(1, 141, width))[:width]
            coded, sizes = hdr.code_planes(planes)
            total += count
            for n in range(count):
                assert coded[n, :sizes[n]].tobytes() == cursor_loop(planes[n]), (alphabet, width, planes[n].tolist())
    assert total >= 10000


def test_sanitising():
    values = np.array([np.nan, -1.0, -0.0, np.inf, -np.inf, 1.0, hdr.FLT_MAX, 1e-40, -1e-40], F)
    expected = np.array([0, 0, 0, hdr.FLT_MAX, 0, 1.0, hdr.FLT_MAX, 1e-40, 0], F)
    assert np.array_equal(hdr.sanitise(values), expected) and not np.signbit(hdr.sanitise(values)[:2]).any()
    # through the half: what overflows it becomes inf and then FLT_MAX, what underflows it zero
    through = hdr.sanitise(np.array([np.nan, -1.0, np.inf, 65519.0, 65520.0, 1e-8, 1.0 / 3.0], F), True)
    assert np.array_equal(through, np.array([0, 0, hdr.FLT_MAX, 65504.0, hdr.FLT_MAX, 0, np.float16(1.0 / 3.0)], F))
    for name, (image, through_half) in hdr_cases.special_inputs().items():
        clean = hdr.sanitise(image[..., :3], through_half)
        assert np.isfinite(clean).all() and (clean >= 0).all()
        # the file is that of the sanitised values, on which the writer is defined
        assert hdr.encode(image, through_half) == hdr.encode(clean), name
        if hdr_cases.reference_available():
            assert hdr.encode(image, through_half) == hdr_cases.reference_file(clean), name
    # one NaN channel leaves the others alone; a pixel of NaNs is black
    quadruples = hdr.rgbe(np.array([[[np.nan, 0.5, 0.25], [np.nan, np.nan, np.nan], [np.inf, 1.0, 0.0]]], F))
    assert quadruples.tolist() == [[[0, 128, 64, 128], [0, 0, 0, 0], [255, 0, 0, 0]]]


def test_through_half_is_the_float_of_the_screenshots_half_split():
    """take_screenshot() renders the frame twice, with frame_bits 1 and 2, joins the low and the high bytes into halves and
    widens them with half_to_float(): through_half names the same floats"""
    import oracle
    lib = capi.load()
    image = np.concatenate([hdr_cases.cases()["through_half_140x2"][0], hdr_cases.cases()["edge_values_46x2"][0][:, :44].repeat(4, axis=1)[:, :140] * F(1e-3)], axis=0)
    image = np.minimum(image, F(60000.0))
    rgba = np.concatenate([image, np.ones(image.shape[:2] + (1,), F)], axis=-1)
    low, high = oracle.encode_half_bits(rgba, 1, False), oracle.encode_half_bits(rgba, 2, False)
    halves = (high[..., :3].astype(np.uint16) << 8) | low[..., :3].astype(np.uint16)
    widened = np.array([lib.half_to_float(int(h)) for h in halves.ravel()], F).reshape(image.shape)
    assert np.array_equal(hdr.sanitise(image, True).view(np.uint32), widened.view(np.uint32))
    assert hdr.encode(image, True) == hdr.encode(widened) != hdr.encode(image)


def test_header_and_narrow_rows():
    assert hdr.header(1920, 1080) == b"#?RADIANCE\n# Written by stb_image_write.h\nFORMAT=32-bit_rle_rgbe\nEXPOSURE=          1.0000000000000\n\n-Y 1080 +X 1920\n"
    image = hdr_cases.cases()["noise_7x2"][0]
    assert hdr.encode(image) == hdr.header(7, 2) + hdr.rgbe(image).tobytes()
    with pytest.raises(ValueError):
        hdr.encode(np.zeros((4, 4), F))
