"""The output encoders of the pass (encode_slab, encode_slab_rgb8, encode_output) against the oracle, byte for byte:
every float of [0, 1] through the sRGB8 encode, the half-float split on every half and its rounding ties and over the
half subnormal and overflow ranges, partial blocks and writes beyond the destination, and whole 1920x1080 frames.
(The CPU side of the same definition: tests/test_output_encoding.py.)"""
import numpy as np
import pytest

import oracle
from helpers import DeviceBuffer, codes_of_range, encoder_specials, half_sweep_chunks, half_test_values, srgb8_by_starts, unorm8
from vulkan_renderer_amd import renderer

pytestmark = pytest.mark.gpu

CHUNK_PIXELS = 1 << 24  # 256 MB of RGBA32F per upload
ONE = 0x3F800000


@pytest.fixture(scope="module")
def starts():
    status, starts = oracle.srgb8_code_starts()
    assert status == 0
    return starts


@pytest.fixture(scope="module")
def encoder():
    """a bare renderer (device and stream, no scene: the encoders need nothing else) and device buffers of one chunk"""
    r = renderer.Renderer()
    buffers = {"in": DeviceBuffer(CHUNK_PIXELS * 16), "rgba": DeviceBuffer(CHUNK_PIXELS * 4), "rgb": DeviceBuffer(CHUNK_PIXELS * 3)}
    yield r, buffers
    for b in buffers.values():
        b.free()
    r.close()


def encode(r, buffers, rgba, frame_bits, output_linear_rgb, packed=False):
    """rgba (uploaded already) -> bytes of encode_slab (RGBA8) or encode_slab_rgb8 (RGB8)"""
    n = len(rgba)
    r.app.screenshot.frame_bits = frame_bits
    try:
        if packed:
            r.encode_slab_rgb8(buffers["in"].ptr.value, buffers["rgb"].ptr.value, n, output_linear_rgb)
            return buffers["rgb"].download((n, 3), np.uint8)
        r.encode_slab(buffers["in"].ptr.value, buffers["rgba"].ptr.value, n, output_linear_rgb)
        return buffers["rgba"].download((n, 4), np.uint8)
    finally:
        r.app.screenshot.frame_bits = 0


def srgb8_all_paths(r, buffers, rgba):
    """the RGBA8 bytes at frame_bits 0; output_linear_rgb 1 and the packed RGB8 form must give the same bytes"""
    buffers["in"].upload(rgba)
    got = encode(r, buffers, rgba, 0, False)
    assert np.array_equal(encode(r, buffers, rgba, 0, True), got), "output_linear_rgb changed sRGB8 bytes"
    assert np.array_equal(encode(r, buffers, rgba, 0, False, packed=True), got[:, :3]), "encode_slab_rgb8 differs from encode_slab"
    assert np.array_equal(encode(r, buffers, rgba, 0, True, packed=True), got[:, :3]), "encode_slab_rgb8 differs from encode_slab"
    return got


def test_srgb8_every_float_of_the_unit_interval(encoder, starts):
    """Every float of [0, 1] in R, G and B (three consecutive bit patterns per pixel) gets the code of the oracle's
    table; alpha carries a third of them (the float at channel i % 3 of pixel i) and gets their UNORM8 in float32."""
    r, buffers = encoder
    wrong = []
    for first in range(0, ONE + 1, 3 * CHUNK_PIXELS):
        pixels = min(CHUNK_PIXELS, -(-(ONE + 1 - first) // 3))
        pixels += -pixels % 4  # (encode_slab_rgb8 takes whole quads; the padding repeats 1.0)
        bits = np.minimum(np.arange(first, first + 3 * pixels, dtype=np.uint32), np.uint32(ONE)).reshape(-1, 3)
        rgba = np.empty((pixels, 4), np.uint32)
        rgba[:, :3] = bits
        rgba[:, 3] = bits[np.arange(pixels), np.arange(pixels) % 3]
        rgba = rgba.view(np.float32)
        got = srgb8_all_paths(r, buffers, rgba)
        rgb = got[:, :3].reshape(-1)
        for i in np.flatnonzero(rgb != codes_of_range(starts, first, 3 * pixels))[:1000]:
            wrong.append((first + int(i), int(rgb[i])))
        alpha = np.flatnonzero(got[:, 3] != unorm8(rgba[:, 3]))
        assert alpha.size == 0, "alpha: %d floats get the wrong byte, e.g. %s" % (
            alpha.size, [(float(rgba[i, 3]).hex(), int(got[i, 3])) for i in alpha[:8]])
    assert not wrong, "%d floats of [0, 1] get another sRGB8 code than the oracle's: %s" % (len(wrong), ", ".join(
        "%s -> %d (oracle %d)" % (float(np.uint32(b).view(np.float32)).hex(), got, int(srgb8_by_starts(np.uint32(b).view(np.float32), starts)[0]))
        for b, got in wrong[:300]))


def test_srgb8_specials(encoder, starts):
    """the specials of tests/helpers.py, the neighbours (+-8 ulps) of every sRGB8 code start and of every UNORM8
    threshold, each in every channel position"""
    r, buffers = encoder
    around = np.arange(-8, 9, dtype=np.int64)
    unorm_thresholds = ((np.arange(1, 256) - 0.5) / 255.0).astype(np.float32).view(np.uint32).astype(np.int64)
    neighbours = np.concatenate([(starts.astype(np.int64)[:, None] + around).ravel(), (unorm_thresholds[:, None] + around).ravel()])
    neighbours = neighbours[(neighbours >= 0) & (neighbours <= ONE)].astype(np.uint32).view(np.float32)
    values = np.concatenate([encoder_specials(), neighbours, -neighbours])
    values = np.append(values, np.full(-len(values) % 4, 0.5, np.float32))
    rgba = np.stack([np.roll(values, j) for j in range(4)], axis=1)  # (value i sits in channel j of pixel i + j)
    got = srgb8_all_paths(r, buffers, rgba)
    expected_rgb = srgb8_by_starts(rgba[:, :3], starts).reshape(-1, 3)
    bad = np.flatnonzero((got[:, :3] != expected_rgb).any(axis=1))
    assert bad.size == 0, [([float(v).hex() for v in rgba[i]], got[i].tolist(), expected_rgb[i].tolist()) for i in bad[:8]]
    assert np.array_equal(got[:, 3], unorm8(rgba[:, 3]))
    assert np.array_equal(got, oracle.encode_srgb8(rgba))


def half_inputs():
    """pixels of the half set and of the sweeps of tests/helpers.py, three values per pixel, in chunks"""
    for values in [half_test_values()] + list(half_sweep_chunks(3 * CHUNK_PIXELS)):
        rgba = np.full((-(-len(values) // 3), 4), 0.5, np.float32)
        rgba[:, :3] = np.append(values, np.zeros(-len(values) % 3, np.float32)).reshape(-1, 3)
        yield values, rgba


def test_half_split(encoder):
    """frame_bits 1 (low byte) and 2 (high byte), both output_linear_rgb: the oracle's bytes exactly; the reassembled
    half is numpy's IEEE conversion (a NaN half with the input's sign for NaN); every byte value occurs"""
    r, buffers = encoder
    seen = {(b, lin): np.zeros(256, bool) for b in (1, 2) for lin in (False, True)}
    for values, rgba in half_inputs():
        buffers["in"].upload(rgba)
        nan = np.isnan(values)
        with np.errstate(over="ignore"):
            ieee = values[~nan].astype(np.float16).view(np.uint16)
        for lin in (False, True):
            split = {}
            for frame_bits in (1, 2):
                got = encode(r, buffers, rgba, frame_bits, lin)
                expected = oracle.encode_half_bits(rgba, frame_bits, lin)
                bad = np.flatnonzero((got != expected).any(axis=1))
                assert bad.size == 0, "frame_bits %d, output_linear_rgb %d: %d pixels differ from the oracle, e.g. %s" % (
                    frame_bits, lin, bad.size, [([float(v).hex() for v in rgba[i, :3]], got[i].tolist(), expected[i].tolist()) for i in bad[:8]])
                seen[(frame_bits, lin)] |= np.bincount(got[:, :3].reshape(-1), minlength=256) > 0
                split[frame_bits] = got
            halves = ((split[2][:, :3].astype(np.uint16) << 8) | split[1][:, :3]).reshape(-1)[:len(values)]
            assert np.array_equal(halves[~nan], ieee), lin
            assert ((halves[nan] & 0x7C00) == 0x7C00).all() and ((halves[nan] & 0x3FF) != 0).all()
            assert np.array_equal(halves[nan] >> 15, (values[nan].view(np.uint32) >> 31).astype(np.uint16))
    # (the high bytes of NaN halves with a payload never occur: the split's NaN is sign | 0x7E00)
    for (frame_bits, lin), s in seen.items():
        missing = np.flatnonzero(~s).tolist()
        assert missing == ([] if frame_bits == 1 else [0x7D, 0x7F, 0xFD, 0xFF]), (frame_bits, lin, missing)


def canary(nbytes):
    return np.random.default_rng(nbytes).integers(0, 256, nbytes, dtype=np.uint8)


def test_partial_blocks_and_bounds(encoder):
    """Pixel counts that are not multiples of the block size write their own pixels and nothing else: the destination
    starts one word into a buffer filled with a canary pattern and has 4 KB of canary past its end."""
    r, buffers = encoder
    largest = 1000003
    rng = np.random.default_rng(5)
    rgba = np.where(rng.random((largest + 1, 4)) < 0.9, rng.random((largest + 1, 4)) * 1.2 - 0.1,
                    np.resize(encoder_specials(), (largest + 1) * 4).reshape(-1, 4)).astype(np.float32)
    buffers["in"].upload(rgba)
    guard = 4096
    for frame_bits in (0, 2):
        full = encode(r, buffers, rgba, frame_bits, False)
        full_rgb = encode(r, buffers, rgba, frame_bits, False, packed=True)
        for count, bytes_per_pixel, packed in [(n, 4, False) for n in (1, 3, 255, 256, 257, largest)] + \
                                              [(n, 3, True) for n in (4, 252, 260, 1028)]:
            size = 4 + count * bytes_per_pixel + guard
            pattern = canary(size)
            destination = DeviceBuffer(size)
            destination.upload(pattern)
            r.app.screenshot.frame_bits = frame_bits
            try:
                call = r.encode_slab_rgb8 if packed else r.encode_slab
                call(buffers["in"].ptr.value, destination.ptr.value + 4, count)
            finally:
                r.app.screenshot.frame_bits = 0
            out = destination.download(size, np.uint8)
            destination.free()
            expected = (full_rgb if packed else full)[:count].reshape(-1)
            assert np.array_equal(out[4:4 + expected.size], expected), (frame_bits, count, packed)
            assert np.array_equal(out[:4], pattern[:4]) and np.array_equal(out[4 + expected.size:], pattern[4 + expected.size:]), \
                "wrote outside its destination: frame_bits %d, %d pixels, packed %s" % (frame_bits, count, packed)
    # encode_slab_rgb8 takes whole quads only: any other count is an error that writes nothing
    for count in (1, 6, 257):
        pattern = canary(4 + count * 3 + guard)
        destination = DeviceBuffer(pattern.size)
        destination.upload(pattern)
        with pytest.raises(RuntimeError):
            r.encode_slab_rgb8(buffers["in"].ptr.value, destination.ptr.value + 4, count)
        assert np.array_equal(destination.download(pattern.size, np.uint8), pattern), count
        destination.free()


@pytest.mark.parametrize("config", [2, 3])
def test_full_size_frames_encode_like_the_oracle(config, big_dataset):
    """1920x1080 frames: encode_output + read_back_encoded and encode_slab_rgb8 of the radiance target give
    oracle.encode_srgb8 of the kernel's own radiance"""
    r = renderer.Renderer()
    renderer.setup_config(r, config, big_dataset, width=1920, height=1080, acceleration_structure="sah_device")
    r.create_targets()
    r.create_pass()
    r.render_visibility()
    r.render()
    radiance = r.read_radiance()
    expected = oracle.encode_srgb8(radiance)
    for lin in (False, True):
        assert np.array_equal(r.read_encoded(output_linear_rgb=lin, frame_bits=0), expected), lin
    packed = DeviceBuffer(1920 * 1080 * 3)
    r.encode_slab_rgb8(r.app.render_targets.radiance, packed.ptr.value, 1920 * 1080)
    r.sync()
    rgb = packed.download((1080, 1920, 3), np.uint8)
    packed.free()
    r.close()
    assert np.array_equal(rgb, expected[..., :3])
