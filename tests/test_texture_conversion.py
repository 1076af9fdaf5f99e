"""The texture converter (include/vkr_texture_conversion.h) without a GPU: the numpy restatement
(vulkan_renderer_amd/texture_conversion.py), which the device matches byte for byte (tests/test_gpu_texture_conversion.py),
against the files the reference's own converter wrote (golden/texture_conversion.npz, made by
golden/make_texture_conversion.py), against the encoders it replaces, and through the unchanged loaders."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

from vulkan_renderer_amd import capi, renderer, synthetic
from vulkan_renderer_amd import texture_conversion as tc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "texture_conversion.npz"))


def cases(golden, formats):
    """(image name, format) of every file of the reference with one of the formats"""
    out = []
    for key in sorted(golden.files):
        if key.startswith("vkt_"):
            name, vk_format = key[4:].rsplit("_", 1)
            if int(vk_format) in formats:
                out.append((name, int(vk_format)))
    return out


def pixels_for(golden, name, vk_format):
    """The pixels the tool converted: its *.hdr loader appends alpha 1 for the four-channel formats"""
    image = golden["input_" + name]
    if vk_format in (97, 109):
        image = np.concatenate([image, np.ones(image.shape[:2] + (1,), np.float32)], -1)
    return image


class Restated:
    """One conversion by the restatement, computed once per module: float levels, 8-bit texels as blocks, encoded blocks"""
    cache = {}

    def __init__(self, image, vk_format):
        self.levels = tc.linear_levels(image, vk_format)
        self.extents = [(level.shape[1], level.shape[0]) for level in self.levels]
        self.payloads = [tc.encode_level(level, vk_format) for level in self.levels]
        self.texels = [tc.blocks_of(tc.quantise(level, vk_format)) for level in self.levels] if tc.FORMATS[vk_format][2] in ("bc1", "bc5") else None

    @classmethod
    def of(cls, golden, name, vk_format):
        if (name, vk_format) not in cls.cache:
            cls.cache[name, vk_format] = cls(pixels_for(golden, name, vk_format), vk_format)
        return cls.cache[name, vk_format]


def squared_error(decoded, texels):
    """per block"""
    difference = decoded.astype(np.int64) - texels.astype(np.int64)
    return (difference * difference).reshape(len(texels), -1).sum(axis=1)


def bc1_blocks(payload):
    return np.frombuffer(payload, np.uint8).reshape(-1, 8)


def bc4_blocks(payload, channel):
    return np.frombuffer(payload, np.uint8).reshape(-1, 2, 8)[:, channel]


# ---- the restatement against the reference's files ------------------------------------------------------------------------

def test_float_formats_equal_the_reference_byte_for_byte(golden):
    """Header, level table, every level and the end marker of the half and float formats: the linear image, the filter
    with its order of additions and the tool's float_to_half are the reference's, operation for operation"""
    found = cases(golden, (90, 97, 106, 109))
    assert len(found) == 8
    for name, vk_format in found:
        restated = Restated.of(golden, name, vk_format)
        assert tc.vkt_bytes(vk_format, restated.extents, restated.payloads) == golden["vkt_%s_%d" % (name, vk_format)].tobytes(), (name, vk_format)


def test_headers_and_level_tables_equal_the_reference(golden):
    found = cases(golden, tc.FORMATS)
    assert len(found) == 28
    for name, vk_format in found:
        reference = golden["vkt_%s_%d" % (name, vk_format)].tobytes()
        restated = Restated.of(golden, name, vk_format)
        mine = tc.vkt_bytes(vk_format, restated.extents, restated.payloads)
        table_end = 32 + 24 * len(restated.extents)
        assert len(mine) == len(reference) and mine[:table_end] == reference[:table_end] and mine[-4:] == reference[-4:], (name, vk_format)


@pytest.mark.parametrize("name,vk_format,expected", [("wide", 131, [(64, 16), (32, 8), (16, 4)]), ("tall", 141, [(16, 64), (8, 32), (4, 16)]),
                                                      ("tiny", 132, [(4, 4)]), ("single", 141, [(4, 4)]), ("strip", 97, [(32, 8), (16, 4), (8, 2), (4, 1)])])
def test_level_counts_are_the_tools(golden, name, vk_format, expected):
    _, levels = tc.read_vkt(golden["vkt_%s_%d" % (name, vk_format)].tobytes())
    image = golden["input_" + name]
    assert [(w, h) for w, h, _ in levels] == expected == tc.level_extents(image.shape[1], image.shape[0], vk_format)


def test_quantised_texels_are_the_ones_the_tool_compressed(golden):
    """The 8-bit texels cannot be read out of a compressed file, but the blocks bound them.
    BC4: stb_dxt stores the largest and the smallest value of a block as its endpoints, so in every block of every
    level the endpoints must be the extremes of the restatement's texels, exactly.  These are the UNORM texels of the
    BC1 files of the same images as well.
    BC1: a block whose texels are all one colour decodes to that colour up to half a step of the endpoint grid (expanded
    five-bit values are 8 or 9 apart, six-bit ones 4 or 5) and one unit for the rounding of the interpolants.
    (The issue asked for every decoded texel of the reference's BC1 blocks to lie within the span of its block's palette
    around the restatement's texel.  The reference's own blocks do not have that property, whatever the texels: the
    palette lies along the block's principal axis and leaves the other directions out, e.g. red 15 ... 247 under a palette
    of red 82 ... 90 in block 217 of the random image, 152 beyond the span.  The floats in front of the quantisation are
    pinned byte for byte by the float formats, which run the same filter; the sRGB texels are pinned by the flat images
    of the next test.)"""
    checked = constant_blocks = 0
    for name, vk_format in cases(golden, (131, 132, 141)):
        restated = Restated.of(golden, name, vk_format)
        _, levels = tc.read_vkt(golden["vkt_%s_%d" % (name, vk_format)].tobytes())
        for texels, (_, _, payload) in zip(restated.texels, levels):
            if vk_format == 141:
                for channel in range(2):
                    blocks = bc4_blocks(payload, channel)
                    assert np.array_equal(blocks[:, 0], texels[:, :, channel].max(axis=1)), (name, channel)
                    assert np.array_equal(blocks[:, 1], texels[:, :, channel].min(axis=1)), (name, channel)
                checked += len(texels)
            else:
                constant = (texels == texels[:, :1]).all(axis=(1, 2))
                decoded = tc.decode_bc1_blocks(bc1_blocks(payload)[constant]).astype(np.int64)
                assert (np.abs(decoded - texels[constant]) <= np.array([5, 3, 5])).all(), (name, vk_format)
                constant_blocks += int(constant.sum())
    assert checked > 1000 and constant_blocks >= 2


def test_srgb_texels_of_flat_images_are_the_ones_the_tool_compressed(golden):
    """The sRGB path - table, filter, sRGB quantisation - pinned through the tool's own blocks.  flat_blocks_131[g] is
    the block the tool makes of sixteen texels (g, g, g): level 0 of a flat 4x4 UNORM image, whose texels are the bytes
    themselves.  The tool's BC1 sRGB file of a flat 16x16 image of every byte value has three levels of flat blocks;
    each must be the block the tool makes of the restatement's texel of that level.  244 of the 256 greys have a block of
    their own, so a texel that is off by one shows in all but a few places."""
    lookup = golden["flat_blocks_131"][:, 0]
    greys = np.arange(256, dtype=np.uint8)
    flat = np.broadcast_to(greys[None, None, :], (4, 4, 256))
    assert np.array_equal(tc.quantise_unorm(flat.astype(np.float32) * (np.float32(1.0) / np.float32(255.0)))[0, 0], greys)
    assert len({bytes(block) for block in lookup}) >= 240
    # one channel per grey level: the filter treats channels alike
    linear = np.ascontiguousarray(np.broadcast_to(tc.srgb_table()[None, None, :], (16, 16, 256)))
    reference = golden["flat_blocks_132"]
    first = 0
    for level in range(3):
        values = linear if level == 0 else tc.filter_level(linear, level)
        texels = tc.quantise_srgb(values)
        assert (texels == texels[:1, :1]).all()
        count = (16 >> level) * (16 >> level) // 16
        expected = lookup[texels[0, 0]]
        assert np.array_equal(reference[:, first:first + count], np.broadcast_to(expected[:, None, :], (256, count, 8))), level
        if level == 0:
            assert np.array_equal(texels[0, 0], greys)
        first += count
    assert first == reference.shape[1] == 21


# ---- quality ------------------------------------------------------------------------------------------------------------------

def test_bc1_is_no_worse_than_the_tool_it_replaces(golden):
    """Summed squared error against the same quantised texels, both decoded by the rule of vkr_decode_bc1_block, per
    image and level: the converter's must not exceed stb_dxt's (margin zero).  Prints the table of DESIGN.md 4.8."""
    failures = []
    for name, vk_format in cases(golden, (131, 132)):
        restated = Restated.of(golden, name, vk_format)
        _, levels = tc.read_vkt(golden["vkt_%s_%d" % (name, vk_format)].tobytes())
        for i, (texels, payload, (_, _, reference)) in enumerate(zip(restated.texels, restated.payloads, levels)):
            mine = int(squared_error(tc.decode_bc1_blocks(bc1_blocks(payload)), texels).sum())
            theirs = int(squared_error(tc.decode_bc1_blocks(bc1_blocks(reference)), texels).sum())
            chain = synthetic.encode_bc1(tc.image_of(texels, *restated.extents[i]))
            old = int(squared_error(tc.decode_bc1_blocks(bc1_blocks(chain)), texels).sum())
            print("%-9s %d level %d: converter %9d  stb_dxt %9d  synthetic.encode_bc1 %9d" % (name, vk_format, i, mine, theirs, old))
            if mine > theirs:
                failures.append((name, vk_format, i, mine, theirs))
    assert not failures, failures


def test_no_bc1_block_is_worse_than_the_synthetic_encoders(golden):
    """Start state A is synthetic.encode_bc1's pair of endpoints and the descent only lowers the error"""
    blocks_checked = 0
    for name, vk_format in cases(golden, (131, 132)):
        restated = Restated.of(golden, name, vk_format)
        for i, (texels, payload) in enumerate(zip(restated.texels, restated.payloads)):
            mine = squared_error(tc.decode_bc1_blocks(bc1_blocks(payload)), texels)
            old = squared_error(tc.decode_bc1_blocks(bc1_blocks(synthetic.encode_bc1(tc.image_of(texels, *restated.extents[i])))), texels)
            assert (mine <= old).all(), (name, vk_format, i)
            blocks_checked += len(texels)
    assert blocks_checked == sum(len(t) for (n, f), r in Restated.cache.items() if f in (131, 132) for t in r.texels)


def test_no_bc4_block_is_worse_than_the_synthetic_encoders_or_the_tools(golden):
    """(max, min) in the eight-value mode, the choice of both, is among the candidates"""
    blocks_checked = 0
    for name, vk_format in cases(golden, (141,)):
        restated = Restated.of(golden, name, vk_format)
        _, levels = tc.read_vkt(golden["vkt_%s_%d" % (name, vk_format)].tobytes())
        for i, (texels, payload, (_, _, reference)) in enumerate(zip(restated.texels, restated.payloads, levels)):
            image = tc.image_of(texels, *restated.extents[i])
            for channel in range(2):
                values = texels[:, :, channel]
                mine = squared_error(tc.decode_bc4_blocks(bc4_blocks(payload, channel)), values)
                theirs = squared_error(tc.decode_bc4_blocks(bc4_blocks(reference, channel)), values)
                old = squared_error(tc.decode_bc4_blocks(np.frombuffer(synthetic.encode_bc4(image[..., channel]), np.uint8).reshape(-1, 8)), values)
                assert (mine <= theirs).all() and (mine <= old).all(), (name, i, channel)
                blocks_checked += len(values)
    assert blocks_checked > 1500


def test_constant_and_two_colour_blocks():
    constant = np.full((1, 16, 3), (200, 17, 96), np.uint8)
    # (two endpoints whose interpolant is nearer than any single 5 / 6 / 5 colour are allowed to win)
    blocks, error = tc.encode_bc1_blocks(constant, return_error=True)
    decoded = tc.decode_bc1_blocks(blocks)
    assert (decoded == decoded[:, :1]).all() and error[0] == squared_error(decoded, constant)[0]
    assert error[0] <= squared_error(tc.decode_bc1_blocks(bc1_blocks(synthetic.encode_bc1(constant.reshape(4, 4, 3)))), constant)[0]
    # black is a colour of the grid: both endpoints equal, all indices 0
    assert tc.encode_bc1_blocks(np.zeros((1, 16, 3), np.uint8)).tolist() == [[0] * 8]
    assert tc.encode_bc4_blocks(constant[:, :, 0]).tolist() == [[200, 200, 0, 0, 0, 0, 0, 0]]
    # two colours that 5 / 6 / 5 bits hold exactly: the block is lossless
    two = np.where((np.arange(16) % 3 == 0)[None, :, None], np.array((255, 0, 132), np.uint8), np.array((0, 255, 0), np.uint8)).astype(np.uint8)
    blocks, error = tc.encode_bc1_blocks(two, return_error=True)
    assert error.tolist() == [0] and np.array_equal(tc.decode_bc1_blocks(blocks), two)


# ---- pieces of the rules ------------------------------------------------------------------------------------------------------

def test_byte_tables_of_the_library_equal_the_restatement():
    """All 256 bit patterns of both tables the device looks bytes up in: the sRGB curve (its constants are binary32
    quotients, 1.0f / 1.055f is not the rounded binary64 quotient) and b * (1 / 255.f)"""
    tables = np.zeros(512, np.float32)
    capi.load().get_texture_conversion_tables(tables.ctypes.data_as(capi.c_float_p))
    assert np.array_equal(tables[:256].view(np.uint32), tc.srgb_table().view(np.uint32))
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(4, axis=2)
    assert np.array_equal(tables[256:].view(np.uint32), tc.linear_image(ramp, 37)[..., 3].reshape(-1).view(np.uint32))
    assert np.array_equal(tables[:256].view(np.uint32), tc.linear_image(ramp, 43)[..., 0].reshape(-1).view(np.uint32))
    assert np.array_equal(tables[256:].view(np.uint32), tc.linear_image(ramp, 43)[..., 3].reshape(-1).view(np.uint32))
    assert tables[0] == 0.0 and tables[255] == 1.0 and tables[511] == 1.0 and (np.diff(tables[:256]) > 0).all()


def test_filter_weights_of_the_library_equal_the_restatement():
    lib = capi.load()
    for level in range(1, tc.MAX_LEVEL + 1):
        extent, weights = tc.filter_weights(level)
        assert lib.get_texture_filter_weights(None, 0, level) == extent == int(np.ceil(np.float32(1.2) * np.float32(1 << level)))
        mine = np.zeros(2 * extent, np.float32)
        assert lib.get_texture_filter_weights(mine.ctypes.data_as(capi.c_float_p), mine.size, level) == extent
        assert np.array_equal(mine.view(np.uint32), weights.view(np.uint32)), level
    assert lib.get_texture_filter_weights(None, 0, 0) == 0 and lib.get_texture_filter_weights(None, 0, tc.MAX_LEVEL + 1) == 0


def test_half_rule_rounds_by_the_first_dropped_bit():
    """Nearest, ties away from zero (numpy's conversion rounds ties to even), over the normal range of the halves"""
    rng = np.random.default_rng(5)
    values = (rng.random(4096) * np.exp2(rng.integers(-14, 15, 4096))).astype(np.float32)
    values = values[values >= 2.0 ** -14]
    ties = (np.arange(1024, 2048, dtype=np.float32) + np.float32(0.5)) * np.float32(2.0 ** -10)
    values = np.concatenate([values, ties, -ties])
    halves = tc.float_to_half(values)
    nearest = values.astype(np.float16).view(np.uint16)
    is_tie = (values.view(np.uint32) & 0x1FFF) == 0x1000
    assert np.array_equal(halves[~is_tie], nearest[~is_tie])
    bits = values[is_tie].view(np.uint32)
    away_from_zero = ((((bits & 0x7FFFFFFF) - (112 << 23)) >> 13) + 1) | ((bits >> 16) & 0x8000)
    assert is_tie.sum() >= 2048 and np.array_equal(halves[is_tie], away_from_zero)
    assert tc.float_to_half(np.array([np.inf, -np.inf, np.nan, 1.0e6, 0.0], np.float32)).tolist() == [0x7C00, 0xFC00, 0x7E00, 0x7C00, 0]


# ---- the C interface ------------------------------------------------------------------------------------------------------------

def test_written_files_load_through_the_unchanged_loader(golden, dataset, tmp_path):
    """write_converted_texture() writes the container; the material loader (vkr_load_texture_rgba8 with
    vkr_decode_bc1_block / vkr_decode_bc5_block) reads it back with the right extents and level counts and decodes every
    block as the Python decoders do"""
    lib = capi.load()
    textures = tmp_path / "textures"
    shutil.copytree(dataset["textures"], textures)
    name = list(synthetic.DEFAULT_MATERIALS)[0]
    written = []
    for suffix, image, vk_format in (("BaseColor", "base", 132), ("Specular", "specular", 131), ("Normal", "normal", 141)):
        restated = Restated.of(golden, image, vk_format)
        texture, keep_alive = tc.converted_texture(vk_format, restated.extents, restated.payloads)
        path = str(textures / ("%s_%s.vkt" % (name, suffix)))
        assert lib.write_converted_texture(C.byref(texture), path.encode()) == 0
        assert open(path, "rb").read() == tc.vkt_bytes(vk_format, restated.extents, restated.payloads)
        written.append((vk_format, restated))
    hs = renderer.HostScene()
    hs.load_scene(dataset["scene"], str(textures))
    materials = hs.app.scene.materials
    names = [materials.material_names[i].decode() for i in range(materials.material_count)]
    descriptors = np.ctypeslib.as_array(materials.host_texture_descriptors, (3 * len(names), 4))
    texels = np.ctypeslib.as_array(materials.host_texels, (materials.texel_count, 4))
    for t, (vk_format, restated) in enumerate(written):
        first, width, height, packed = (int(v) for v in descriptors[3 * names.index(name) + t])
        assert (width, height) == (64, 64) and packed & 0xFFFF == len(restated.extents) == 5 and packed >> 16 == (vk_format == 132)
        for (w, h), payload in zip(restated.extents, restated.payloads):
            expected = np.zeros((h, w, 4), np.uint8)
            expected[..., 3] = 255
            if vk_format == 141:
                for channel in range(2):
                    expected[..., channel] = tc.image_of(tc.decode_bc4_blocks(bc4_blocks(payload, channel))[:, :, None], w, h)[..., 0]
            else:
                expected[..., :3] = tc.image_of(tc.decode_bc1_blocks(bc1_blocks(payload)), w, h)
                # (the definitions of synthetic.py, block by block)
                assert np.array_equal(expected[:4, :4], synthetic.decode_bc1_block(payload[:8]))
            assert np.array_equal(texels[first:first + w * h].reshape(h, w, 4), expected), (vk_format, w, h)
            first += w * h
    hs.close()
    empty = capi.ConvertedTexture()
    assert lib.write_converted_texture(C.byref(empty), str(tmp_path / "none.vkt").encode()) == 1
    assert lib.write_converted_texture(C.byref(texture), str(tmp_path / "missing" / "directory.vkt").encode()) == 1


def test_refusals_return_1_with_a_zeroed_struct(capfd):
    lib = capi.load()
    assert C.sizeof(capi.ConvertedTexture) == 16 + 8 + 2 * 32 * 8 + 8
    pixels = np.zeros((8, 8, 4), np.uint8)
    # (what the library printed before this test is still in the C library's buffer)
    C.CDLL(None).fflush(None)
    capfd.readouterr()

    def refused(width, height, channels, vk_format):
        texture = capi.ConvertedTexture()
        texture.mipmap_count, texture.payload_size = 7, 99
        status = lib.convert_texture(C.byref(texture), None, pixels.ctypes.data, width, height, channels, vk_format)
        C.CDLL(None).fflush(None)
        printed = capfd.readouterr().out
        return status == 1 and bytes(texture) == bytes(C.sizeof(texture)) and printed.count("\n") == 1

    assert refused(8, 8, 4, 132)       # no device: there is no host build of the converter
    assert refused(8, 8, 4, 133)       # BC1 with alpha is not written
    assert refused(8, 8, 4, 0)
    assert refused(8, 8, 2, 131) and refused(8, 8, 1, 141) and refused(8, 8, 3, 37) and refused(8, 8, 3, 109)
    assert refused(8, 6, 4, 37) and refused(0, 8, 4, 37) and refused(8192, 8, 4, 37)
    assert refused(8, 2, 4, 131) and refused(2, 2, 4, 141) and refused(1, 2, 4, 132)
    for arguments in ((8, 6, 37), (8, 2, 131), (8, 8, 133), (8192, 8, 37)):
        with pytest.raises(ValueError):
            tc.level_extents(*arguments)
    with pytest.raises(ValueError):
        tc.linear_image(pixels[..., :2], 131)


def test_command_line_prints_its_usage():
    assert tc.main([]) == 1 and tc.main(["133", "a.npy", "b.vkt"]) == 1 and tc.main(["132", "stray", "a.npy", "b.vkt"]) == 1
