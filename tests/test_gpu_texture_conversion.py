"""Textures converted on the GPU (include/vkr_texture_conversion.h convert_texture, csrc/texture_conversion.hip) against
their numpy restatement (vulkan_renderer_amd/texture_conversion.py, pinned by tests/test_texture_conversion.py) in every
byte, and a frame shaded with them against the CPU oracle in every bit."""
import functools
import os

import numpy as np
import pytest

import golden_cases
from helpers import oracle_render
from vulkan_renderer_amd import renderer, synthetic
from vulkan_renderer_amd import texture_conversion as tc

pytestmark = pytest.mark.gpu

BLOCK_FORMATS, FLOAT_FORMATS = (131, 132, 141), (90, 97, 106, 109)


@pytest.fixture(scope="module")
def device():
    r = renderer.Renderer()
    yield r
    r.close()


@functools.lru_cache(maxsize=None)
def byte_image(width, height):
    """Random colours over a smooth ramp: blocks of wide and of narrow range, and no two levels alike"""
    rng = np.random.default_rng(1000 * width + height)
    ramp = np.linspace(0.0, 160.0, width)[None, :, None] + np.linspace(0.0, 40.0, height)[:, None, None]
    image = np.clip(ramp + rng.integers(0, 56, (height, width, 4)), 0, 255).astype(np.uint8)
    image[: height // 2, : width // 2] = rng.integers(0, 256, (height // 2, width // 2, 4))
    return image


@functools.lru_cache(maxsize=None)
def float_image(width, height):
    """Many binades, values in the subnormal range of the halves and below it, beyond their largest, both signs"""
    rng = np.random.default_rng(7 * width + height)
    image = (rng.random((height, width, 4)) * np.exp2(rng.integers(-8, 6, (height, width, 1)))).astype(np.float32)
    image[0, :8] *= np.float32(1.0e-6)
    image[1, :8] *= np.float32(1.0e-9)
    image[2, :8] *= np.float32(3.0e4)
    image[3, :8] *= np.float32(-1.0)
    return image


@functools.lru_cache(maxsize=None)
def restated(vk_format, width, height):
    image = float_image(width, height) if tc.takes_float(vk_format) else byte_image(width, height)
    return tc.convert(image, vk_format)


def differing_bytes(got, expected):
    assert [len(p) for p in got] == [len(p) for p in expected]
    return [int((np.frombuffer(a, np.uint8) != np.frombuffer(b, np.uint8)).sum()) for a, b in zip(got, expected)]


# 64x64: the smallest size at which the footprint of a level wraps round the image more than once and a level has lanes
# of more than one wave; 64x16 and 16x64 for the level count and unequal masks; 8x8, 4x4 and 1x1 down to the single block
@pytest.mark.parametrize("width,height", [(64, 64), (64, 16), (16, 64), (8, 8), (4, 4), (1, 1)])
@pytest.mark.parametrize("vk_format", BLOCK_FORMATS)
def test_block_formats_equal_the_restatement(device, vk_format, width, height):
    extents, payloads = device.convert_texture(byte_image(width, height), vk_format)
    expected_extents, expected = restated(vk_format, width, height)
    assert extents == expected_extents == tc.level_extents(width, height, vk_format)
    differing = differing_bytes(payloads, expected)
    assert not any(differing), "bytes that differ per level: %r" % (differing,)


@pytest.mark.parametrize("width,height", [(32, 8), (64, 64)])
@pytest.mark.parametrize("vk_format", FLOAT_FORMATS + (37, 43))
def test_formats_without_blocks_equal_the_restatement(device, vk_format, width, height):
    image = float_image(width, height) if tc.takes_float(vk_format) else byte_image(width, height)
    extents, payloads = device.convert_texture(image, vk_format)
    expected_extents, expected = restated(vk_format, width, height)
    assert extents == expected_extents and len(extents) == min(width, height).bit_length()
    differing = differing_bytes(payloads, expected)
    assert not any(differing), "bytes that differ per level: %r" % (differing,)
    if vk_format == 109:
        # (level 0 is the input)
        assert payloads[0] == np.ascontiguousarray(image).tobytes()


def test_srgb_levels_of_a_large_image_equal_the_restatement(device):
    """1024x1024 as RGBA8 sRGB, levels 0 to 2 (the restatement of the higher ones takes minutes): three million values
    through the sRGB table, the filter and the quantisation.  At this size a table that is off by one unit in the last
    place shows in about a dozen bytes; at 64x64 the rounding to 8 bits hides it."""
    rng = np.random.default_rng(1024)
    image = rng.integers(0, 256, (1024, 1024, 4), dtype=np.uint8)
    extents, payloads = device.convert_texture(image, 43)
    assert extents == tc.level_extents(1024, 1024, 43) and len(extents) == 11
    linear = tc.linear_image(image, 43)
    assert payloads[0] == image.tobytes()
    for level in (1, 2):
        expected = tc.encode_level(tc.filter_level(linear, level), 43)
        differing = differing_bytes([payloads[level]], [expected])
        assert differing == [0], "level %d: %d bytes differ" % (level, differing[0])


def test_halves_of_infinity_and_nan(device):
    """(one texel, one level: a NaN in a larger image would fill every level above 0)"""
    texel = np.array([[[np.inf, -np.inf, np.nan, -0.0]]], np.float32)
    extents, payloads = device.convert_texture(texel, 97)
    assert extents == [(1, 1)] and np.frombuffer(payloads[0], np.uint16).tolist() == [0x7C00, 0xFC00, 0x7E00, 0x8000]
    assert payloads == tc.convert(texel, 97)[1]


@pytest.mark.parametrize("vk_format", BLOCK_FORMATS)
def test_constant_and_two_colour_images(device, vk_format):
    """c0 == c1 with all indices 0, and blocks whose descent starts at the optimum or next to it"""
    constant = np.broadcast_to(np.array((0, 0, 0), np.uint8), (8, 8, 3))
    grey = np.broadcast_to(np.array((201, 17, 96), np.uint8), (8, 8, 3))
    two = np.where(((np.arange(16)[:, None] // 3 + np.arange(16)[None, :] // 5) % 2 == 0)[..., None], np.array((250, 12, 130), np.uint8), np.array((7, 240, 3), np.uint8)).astype(np.uint8)
    for image in (constant, grey, two):
        extents, payloads = device.convert_texture(image, vk_format)
        assert (extents, payloads) == tc.convert(image, vk_format)
    if vk_format != 141:
        assert device.convert_texture(constant, vk_format)[1][0] == bytes(32)


def test_more_channels_than_the_format_has_are_dropped(device):
    image = byte_image(16, 64)
    assert device.convert_texture(image, 141) == device.convert_texture(image[..., :2], 141)
    assert device.convert_texture(image, 132) == device.convert_texture(image[..., :3], 132)
    with pytest.raises(RuntimeError):
        device.convert_texture(image[..., :2], 131)


@pytest.fixture(scope="module")
def converted_dataset(device, tmp_path_factory):
    """The textured data set of the golden frames with every material texture converted on the device from
    procedural_textures(): BC1 sRGB base colour, BC1 UNORM specular, BC5 normal"""
    dataset = synthetic.write_dataset(str(tmp_path_factory.mktemp("converted")), **golden_cases.TEXTURED_DATASET)
    for index, name in enumerate(synthetic.DEFAULT_MATERIALS):
        images = synthetic.procedural_textures(golden_cases.TEXTURED_DATASET["texture_size"], seed=3 + index)
        for image, suffix, vk_format in zip(images, ("BaseColor", "Specular", "Normal"), (132, 131, 141)):
            path = os.path.join(dataset["textures"], "%s_%s.vkt" % (name, suffix))
            extents, payloads = device.convert_texture(image, vk_format, path=path)
            assert open(path, "rb").read() == tc.vkt_bytes(vk_format, extents, payloads)
            if index == 0:
                assert (extents, payloads) == tc.convert(image, vk_format)
    return dataset


def test_a_frame_with_converted_textures_equals_the_oracle_bit_for_bit(converted_dataset):
    """The files go through the unchanged loader into the unchanged pass; the oracle shades from the same files"""
    case = golden_cases.TEXTURED_CASES[1]
    r = renderer.Renderer(arithmetic="libm")
    golden_cases.apply_case(r, case, converted_dataset)
    materials = r.app.scene.materials
    descriptors = np.ctypeslib.as_array(materials.host_texture_descriptors, (9, 4))
    assert materials.textured == 1 and (descriptors[:, 1:3] == 32).all() and ((descriptors[:, 3] & 0xFFFF) == 4).all()
    r.create_targets()
    r.create_pass()
    r.render_visibility()
    r.render()
    image = r.read_radiance()
    cpu, _, _ = oracle_render(r, visibility=r.read_visibility(), math_mode=renderer.ORACLE_MATH_MODE["libm"])
    r.close()
    assert not np.isnan(image).any() and image[..., :3].max() > 0.0
    assert np.array_equal(image[..., :3].view(np.uint32), cpu[..., :3].astype(np.float32).view(np.uint32))


def test_conversions_queued_behind_a_frame_in_flight(converted_dataset):
    """Two conversions behind each other and behind frames that have not finished give the bytes of each alone, and
    leave the frames as they are"""
    case = golden_cases.TEXTURED_CASES[1]
    r = renderer.Renderer(arithmetic="libm", frames_in_flight=2)
    golden_cases.apply_case(r, case, converted_dataset)
    r.create_targets()
    r.create_pass()
    r.render_visibility()
    r.render()
    alone = r.read_radiance()
    first_alone, second_alone = r.convert_texture(byte_image(64, 16), 132), r.convert_texture(byte_image(16, 64), 141)
    r.sync()
    for _ in range(3):
        r.render()
    second, first = r.convert_texture(byte_image(16, 64), 141), r.convert_texture(byte_image(64, 16), 132)
    image = r.read_radiance()
    r.close()
    assert first == first_alone and second == second_alone
    assert first == restated(132, 64, 16) and second == restated(141, 16, 64)
    assert np.array_equal(image.view(np.uint32), alone.view(np.uint32))
