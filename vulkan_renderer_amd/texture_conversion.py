"""The texture converter of include/vkr_texture_conversion.h restated in numpy: convert() gives the bytes that
convert_texture() computes on the device, level by level (the header has the rules; the names below are its names).

    python -m vulkan_renderer_amd.texture_conversion FORMAT INPUT OUTPUT

converts INPUT on the device and writes OUTPUT (*.vkt), with the argument order of the reference's
tools/texture_conversion.  INPUT is a .npy file (uint8 or float32, height x width x channels); other image types are
read with PIL where it can be imported."""
import ctypes as C
import math
import struct
import sys

import numpy as np

from . import capi

# format: (channels, bits per pixel, kind, sRGB)
FORMATS = {
    37: (4, 32, "rgba8", False), 43: (4, 32, "rgba8", True),
    90: (3, 48, "half", False), 97: (4, 64, "half", False), 106: (3, 96, "float", False), 109: (4, 128, "float", False),
    131: (3, 4, "bc1", False), 132: (3, 4, "bc1", True), 141: (2, 8, "bc5", False),
}
MAX_LEVEL = 12
# (level, j, bits): the weights for which the reference's expf() and (float) exp() disagree; the rule takes expf's bits
WEIGHT_EXCEPTIONS = ((11, 708, 0x3DD162FB), (11, 1476, 0x3EF9C792), (11, 1626, 0x3F18F0D1), (11, 2150, 0x3F6E95E1),
                     (11, 2765, 0x3F6E95E1), (11, 3289, 0x3F18F0D1), (11, 3439, 0x3EF9C792), (11, 4207, 0x3DD162FB),
                     (12, 109, 0x3C5D9AD4), (12, 1833, 0x3E2E7282), (12, 3922, 0x3F5501DF), (12, 5909, 0x3F5501DF),
                     (12, 7998, 0x3E2E7282), (12, 9722, 0x3C5D9AD4))
f32 = np.float32


def takes_float(vk_format):
    return FORMATS[vk_format][2] in ("half", "float")


def powf(x, y):
    """powf of csrc/glibc_math.h on an array"""
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    capi.load().evaluate_texture_conversion_powf(out.ctypes.data_as(capi.c_float_p), x.ctypes.data_as(capi.c_float_p), float(y), x.size)
    return out


def level_extents(width, height, vk_format):
    """[(width, height)] of the levels, after the 1x1 -> 4x4 rule of the block formats; raises ValueError for what
    convert_texture() refuses"""
    if vk_format not in FORMATS:
        raise ValueError("unknown format %r" % (vk_format,))
    block = FORMATS[vk_format][2] in ("bc1", "bc5")
    for extent in (width, height):
        if extent < 1 or extent & (extent - 1) or extent > 1 << MAX_LEVEL:
            raise ValueError("extent %dx%d is not a power of two up to %d" % (width, height, 1 << MAX_LEVEL))
    if block and (width, height) == (1, 1):
        return [(4, 4)]
    count = min(width.bit_length(), height.bit_length())
    if block:
        if width < 4 or height < 4:
            raise ValueError("extent %dx%d is below 4x4" % (width, height))
        count -= 2
    return [(width >> i, height >> i) for i in range(count)]


def srgb_table():
    """The linear value of every sRGB byte.  The constants are quotients of binary32 numbers, as in C: 1.0f / 1.055f and
    0.055f / 1.055f are one unit in the last place away from the binary64 quotients rounded to binary32"""
    s = np.arange(256, dtype=np.float32) * (f32(1.0) / f32(255.0))
    curve = powf(s * (f32(1.0) / f32(1.055)) + f32(0.055) / f32(1.055), f32(2.4))
    return np.where(s <= f32(0.04045), s * (f32(1.0) / f32(12.92)), curve).astype(np.float32)


def linear_image(pixels, vk_format):
    channels, _, kind, srgb = FORMATS[vk_format]
    pixels = np.asarray(pixels)
    if pixels.ndim != 3 or pixels.shape[2] < channels:
        raise ValueError("the image needs at least %d channels" % channels)
    pixels = pixels[..., :channels]
    if kind in ("half", "float"):
        return np.ascontiguousarray(pixels, np.float32)
    if pixels.dtype != np.uint8:
        raise ValueError("format %d takes uint8 pixels" % vk_format)
    linear = pixels.astype(np.float32) * (f32(1.0) / f32(255.0))
    if srgb:
        linear[..., :3] = srgb_table()[pixels[..., :3]]
    return linear


def filter_weights(level):
    """(E, the 2 E normalised weights) of a level above 0"""
    stride = 1 << level
    sigma = f32(0.4) * f32(stride)
    g = f32(-0.5) / (sigma * sigma)
    extent = int(np.ceil(f32(3.0) * sigma))
    center = f32(extent) - f32(0.5)
    d = np.arange(2 * extent, dtype=np.float32) - center
    # (math.exp is the C library's exp, as in the host code)
    weights = np.array([math.exp(float(a)) for a in (g * d) * d]).astype(np.float32)
    for exception_level, j, bits in WEIGHT_EXCEPTIONS:
        if exception_level == level:
            weights[j] = np.uint32(bits).view(np.float32)
    total = f32(0.0)
    for w in weights:
        total = f32(total + w)
    return extent, weights * (f32(1.0) / total)


def filter_level(linear, level):
    """Level `level` > 0 of the chain: the sequential sum, k outer and j inner, over the whole level at once"""
    height, width, _ = linear.shape
    extent, weights = filter_weights(level)
    stride = 1 << level
    xs = np.arange(width >> level) * stride + stride // 2 - extent
    ys = np.arange(height >> level) * stride + stride // 2 - extent
    out = np.zeros((height >> level, width >> level, linear.shape[2]), np.float32)
    for k in range(2 * extent):
        rows = linear[(ys + k) & (height - 1)]
        for j in range(2 * extent):
            out += (weights[j] * weights[k]) * rows[:, (xs + j) & (width - 1)]
    return out


def roundf(x):
    """C's roundf: halves away from zero"""
    magnitude = np.abs(x)
    whole = np.trunc(magnitude)
    return np.copysign(whole + (magnitude - whole >= f32(0.5)), x).astype(np.float32)


def quantise_unorm(v):
    return np.clip(roundf(v * f32(255.0)), 0.0, 255.0).astype(np.uint8)


def quantise_srgb(v):
    v = np.where(v < 0.0, f32(0.0), v).astype(np.float32)
    s = np.where(v <= f32(0.0031308), f32(12.92) * v, f32(1.055) * powf(v, f32(1.0) / f32(2.4)) - f32(0.055)).astype(np.float32)
    return np.clip(roundf(s * f32(255.0)), 0.0, 255.0).astype(np.uint8)


def quantise(level, vk_format):
    """The 8-bit texels of a level of the formats that have them (the texels the block encoders see)"""
    _, _, _, srgb = FORMATS[vk_format]
    texels = quantise_unorm(level)
    if srgb:
        texels[..., :3] = quantise_srgb(level[..., :3])
    return texels


def float_to_half(values):
    """uint16 patterns by the rule of the reference tool: round by the first dropped bit, ties away from zero"""
    u = np.ascontiguousarray(values, np.float32).view(np.uint32).copy()
    sign = u & np.uint32(0x80000000)
    u ^= sign
    special = u >= 0x7F800000
    special_half = np.where(u > 0x7F800000, 0x7E00, 0x7C00).astype(np.uint32)
    u &= np.uint32(0xFFFFF000)
    with np.errstate(under="ignore"):
        u = (u.view(np.float32) * np.uint32(15 << 23).view(np.float32)).view(np.uint32)
    u = np.minimum(u + np.uint32(0x1000), np.uint32(31 << 23))
    return (np.where(special, special_half, u >> 13) | (sign >> 16)).astype(np.uint16)


# ---- blocks ---------------------------------------------------------------------------------------------------------

def blocks_of(texels):
    """(height, width, channels) -> (blocks, 16, channels), blocks row by row, texel number 4 y + x"""
    height, width, channels = texels.shape
    return texels.reshape(height // 4, 4, width // 4, 4, channels).transpose(0, 2, 1, 3, 4).reshape(-1, 16, channels)


def image_of(blocks, width, height):
    """The inverse of blocks_of()"""
    channels = blocks.shape[2]
    return blocks.reshape(height // 4, width // 4, 4, 4, channels).transpose(0, 2, 1, 3, 4).reshape(height, width, channels)


def bc4_palette(e0, e1):
    """(N, 8) values of decode_bc4_block"""
    e0, e1 = e0.astype(np.int64), e1.astype(np.int64)
    eight = [e0, e1] + [((7 - i) * e0 + i * e1 + 3) // 7 for i in range(1, 7)]
    six = [e0, e1] + [((5 - i) * e0 + i * e1 + 2) // 5 for i in range(1, 5)] + [np.zeros_like(e0), np.full_like(e0, 255)]
    return np.where((e0 > e1)[:, None], np.stack(eight, 1), np.stack(six, 1))


def bc4_error(values, e0, e1):
    """values (N, 16): (error (N,), indices (N, 16)) of the pair"""
    d = (values[:, :, None].astype(np.int64) - bc4_palette(e0, e1)[:, None, :]) ** 2
    return d.min(axis=2).sum(axis=1), d.argmin(axis=2)


def encode_bc4_blocks(values):
    """(N, 16) uint8 -> (N, 8) uint8"""
    values = np.asarray(values).astype(np.int64)
    low, high = values.min(axis=1), values.max(axis=1)
    best_error = np.full(len(values), np.iinfo(np.int64).max)
    best_key = np.zeros(len(values), np.int64)
    for dh in range(5):
        for dl in range(5):
            hi, lo = high - dh, low + dl
            valid = (hi >= low) & (lo <= high)
            for e0, e1 in ((hi, lo), (lo, hi)):
                e0, e1 = np.where(valid, e0, high), np.where(valid, e1, low)
                error, _ = bc4_error(values, e0, e1)
                key = (e0 << 8) | e1
                better = valid & ((error < best_error) | ((error == best_error) & (key < best_key)))
                best_error, best_key = np.where(better, error, best_error), np.where(better, key, best_key)
    e0, e1 = best_key >> 8, best_key & 255
    _, indices = bc4_error(values, e0, e1)
    packed = e0 | (e1 << 8) | ((indices.astype(np.int64) << (3 * np.arange(16) + 16)).sum(axis=1))
    return packed.astype("<u8").view(np.uint8).reshape(-1, 8)


def bc1_colours(e):
    """(N, 6) states -> (c0, c1) as stored: swapped where c0 < c1"""
    e = e.astype(np.int64)
    c0 = (e[:, 0] << 11) | (e[:, 1] << 5) | e[:, 2]
    c1 = (e[:, 3] << 11) | (e[:, 4] << 5) | e[:, 5]
    return np.maximum(c0, c1), np.minimum(c0, c1)


def bc1_palette(c0, c1):
    """(N, 4, 3): the four-colour palette of vkr_decode_bc1_block"""
    def expand(c):
        r, g, b = c >> 11, (c >> 5) & 63, c & 31
        return np.stack([(r << 3) | (r >> 2), (g << 2) | (g >> 4), (b << 3) | (b >> 2)], -1)
    p0, p1 = expand(c0), expand(c1)
    return np.stack([p0, p1, (2 * p0 + p1 + 1) // 3, (p0 + 2 * p1 + 1) // 3], 1)


def bc1_error(texels, e):
    """texels (N, 16, 3), e (N, 6): (E (N,), indices (N, 16))"""
    palette = bc1_palette(*bc1_colours(e))
    d = ((texels[:, :, None, :].astype(np.int64) - palette[:, None, :, :]) ** 2).sum(axis=3)
    return d.min(axis=2).sum(axis=1), d.argmin(axis=2)


def _normalise(v):
    largest = np.abs(v).max(axis=1)
    bits = ((largest[:, None] >> np.arange(48)) > 0).sum(axis=1)
    return v >> np.maximum(bits - 10, 0)[:, None]


def _round_565(rgb):
    return np.stack([(31 * rgb[:, 0] + 127) // 255, (63 * rgb[:, 1] + 127) // 255, (31 * rgb[:, 2] + 127) // 255], 1)


def bc1_start_states(texels):
    """(3, N, 6): the start states A, B and C"""
    t = texels.astype(np.int64)
    n = np.arange(len(t))
    luminance = t @ np.array([2, 5, 1])
    bright, dark = t[n, luminance.argmax(axis=1)], t[n, luminance.argmin(axis=1)]
    a = np.concatenate([bright >> np.array([3, 2, 3]), dark >> np.array([3, 2, 3])], 1)
    S = t.sum(axis=1)
    P = np.einsum("nia,nib->nab", t, t)
    cov = 16 * P - S[:, :, None] * S[:, None, :]
    diagonal = np.stack([cov[:, 0, 0], cov[:, 1, 1], cov[:, 2, 2]], 1)
    v = _normalise(cov[n, diagonal.argmax(axis=1)])
    for _ in range(4):
        v = _normalise(np.einsum("nab,nb->na", cov, v))
    projection = np.einsum("nic,nc->ni", t, v)
    b = np.concatenate([_round_565(t[n, projection.argmax(axis=1)]), _round_565(t[n, projection.argmin(axis=1)])], 1)
    c = np.concatenate([_round_565(t.max(axis=1)), _round_565(t.min(axis=1))], 1)
    return np.stack([a, b, c])


def encode_bc1_blocks(texels, return_error=False):
    """(N, 16, 3) uint8 -> (N, 8) uint8"""
    texels = np.asarray(texels)
    count = len(texels)
    e = bc1_start_states(texels).reshape(3 * count, 6)
    t = np.concatenate([texels] * 3)
    error, _ = bc1_error(t, e)
    limits = np.array([31, 63, 31, 31, 63, 31])
    for _ in range(32):
        accepted = False
        for step in (1, 2):
            for k in range(6):
                for s in (-step, step):
                    trial = e.copy()
                    trial[:, k] += s
                    in_range = (trial[:, k] >= 0) & (trial[:, k] <= limits[k])
                    trial[:, k] = np.clip(trial[:, k], 0, limits[k])
                    trial_error, _ = bc1_error(t, trial)
                    accept = in_range & (trial_error < error)
                    e[accept], error[accept] = trial[accept], trial_error[accept]
                    accepted = accepted or bool(accept.any())
        # (a block without an acceptance in this round is at a fixed point: further rounds leave it as it is)
        if not accepted:
            break
    e, error = e.reshape(3, count, 6), error.reshape(3, count)
    winner = error.argmin(axis=0)
    e, error = e[winner, np.arange(count)], error[winner, np.arange(count)]
    _, indices = bc1_error(texels, e)
    c0, c1 = bc1_colours(e)
    packed = c0 | (c1 << 16) | ((indices.astype(np.int64) << (2 * np.arange(16) + 32)).sum(axis=1))
    blocks = packed.astype("<u8").view(np.uint8).reshape(-1, 8)
    return (blocks, error) if return_error else blocks


def decode_bc1_blocks(blocks):
    """(N, 8) uint8 -> (N, 16, 3) by the rule of vkr_decode_bc1_block (RGB formats: no transparent entry)"""
    packed = np.ascontiguousarray(blocks, np.uint8).view("<u8").reshape(-1).astype(np.int64)
    c0, c1 = packed & 0xFFFF, (packed >> 16) & 0xFFFF
    four = bc1_palette(c0, c1)
    three = four.copy()
    three[:, 2] = (four[:, 0] + four[:, 1] + 1) // 2
    three[:, 3] = 0
    palette = np.where((c0 > c1)[:, None, None], four, three)
    indices = (packed[:, None] >> (2 * np.arange(16) + 32)) & 3
    return palette[np.arange(len(packed))[:, None], indices].astype(np.uint8)


def decode_bc4_blocks(blocks):
    """(N, 8) uint8 -> (N, 16)"""
    packed = np.ascontiguousarray(blocks, np.uint8).view("<u8").reshape(-1)
    palette = bc4_palette((packed & np.uint64(255)).astype(np.int64), ((packed >> np.uint64(8)) & np.uint64(255)).astype(np.int64))
    indices = ((packed[:, None] >> (3 * np.arange(16, dtype=np.uint64) + np.uint64(16))) & np.uint64(7)).astype(np.int64)
    return palette[np.arange(len(packed))[:, None], indices].astype(np.uint8)


# ---- the whole conversion ---------------------------------------------------------------------------------------------

def linear_levels(pixels, vk_format):
    """The float levels, after the 1x1 -> 4x4 rule"""
    linear = linear_image(pixels, vk_format)
    extents = level_extents(linear.shape[1], linear.shape[0], vk_format)
    if extents[0] != (linear.shape[1], linear.shape[0]):
        linear = np.ascontiguousarray(np.broadcast_to(linear[:1, :1], (4, 4, linear.shape[2])))
    return [linear] + [filter_level(linear, i) for i in range(1, len(extents))]


def encode_level(level, vk_format):
    """The payload bytes of one float level"""
    kind = FORMATS[vk_format][2]
    if kind == "float":
        return level.tobytes()
    if kind == "half":
        return float_to_half(level).tobytes()
    texels = quantise(level, vk_format)
    if kind == "rgba8":
        return texels.tobytes()
    blocks = blocks_of(texels)
    if kind == "bc1":
        return encode_bc1_blocks(blocks).tobytes()
    red, green = encode_bc4_blocks(blocks[:, :, 0]), encode_bc4_blocks(blocks[:, :, 1])
    return np.concatenate([red, green], 1).tobytes()


def convert(pixels, vk_format):
    """(extents, payloads) of convert_texture(): [(width, height)] and the bytes of every level"""
    levels = linear_levels(pixels, vk_format)
    return [(level.shape[1], level.shape[0]) for level in levels], [encode_level(level, vk_format) for level in levels]


def vkt_bytes(vk_format, extents, payloads):
    """The file write_converted_texture() writes"""
    out = [struct.pack("<iiiiiiQ", 0xBC1BC1, 1, len(payloads), extents[0][0], extents[0][1], vk_format, sum(map(len, payloads)))]
    offset = 0
    for (width, height), data in zip(extents, payloads):
        out.append(struct.pack("<iiQQ", width, height, len(data), offset))
        offset += len(data)
    return b"".join(out + list(payloads) + [struct.pack("<I", 0xE0FE0F)])


def read_vkt(data):
    """bytes of a *.vkt -> (format, [(width, height, payload bytes)])"""
    marker, version, count, _, _, vk_format, size = struct.unpack_from("<iiiiiiQ", data, 0)
    table = [struct.unpack_from("<iiQQ", data, 32 + 24 * m) for m in range(count)]
    start = 32 + 24 * count
    if marker != 0xBC1BC1 or version != 1 or struct.unpack_from("<I", data, start + size)[0] != 0xE0FE0F:
        raise ValueError("not a *.vkt file")
    return vk_format, [(w, h, bytes(data[start + o:start + o + s])) for w, h, s, o in table]


def converted_texture(vk_format, extents, payloads):
    """A capi.ConvertedTexture over the given levels (the payload is owned by Python: do not free it from C) and the
    buffer that keeps it alive"""
    texture = capi.ConvertedTexture()
    texture.format, texture.mipmap_count, (texture.width, texture.height) = vk_format, len(payloads), extents[0]
    offset = 0
    for i, data in enumerate(payloads):
        texture.mipmap_sizes[i], texture.mipmap_offsets[i] = len(data), offset
        offset += len(data)
    texture.payload_size = offset
    buffer = C.create_string_buffer(b"".join(payloads), offset)
    texture.payload = C.cast(buffer, C.POINTER(C.c_uint8))
    return texture, buffer


def load_image(path, vk_format):
    if path.endswith(".npy"):
        image = np.load(path)
    else:
        try:
            from PIL import Image
        except ImportError:
            raise SystemExit("%s is not a .npy file and PIL cannot be imported." % path)
        image = np.asarray(Image.open(path))
    if image.ndim == 2:
        image = image[..., None]
    return np.ascontiguousarray(image, np.float32 if takes_float(vk_format) else np.uint8)


def main(argv):
    if len(argv) != 3 or not argv[0].lstrip("-").isdigit() or int(argv[0]) not in FORMATS:
        print("Usage: python -m vulkan_renderer_amd.texture_conversion <vk_format> <input_file_path> <output_file_path>")
        print("vk_format is one of " + ", ".join(str(f) for f in sorted(FORMATS)) + " (VkFormat values).")
        return 1
    from . import renderer
    vk_format = int(argv[0])
    r = renderer.Renderer(hip_device=0)
    try:
        r.convert_texture(load_image(argv[1], vk_format), vk_format, path=argv[2])
    finally:
        r.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
