"""Feature buffers (include/vkr_feature_buffers.h) restated in numpy, byte for byte, and a command line that writes them.

The shading data themselves - position, normal, outgoing, albedo, F0, roughness - are not restated here: they are the pass's
get_shading_data(), whose specification is the CPU oracle's oracle_shading_data().  What this module states are the rules
that the header adds on top of them: the distance, the reprojection, what a pixel with nothing visible holds, and the five
previews.  Everything is binary32 with each operation rounded on its own, which is what numpy does with float32 arrays.

    python -m vulkan_renderer_amd.feature_buffers DATASET [--config N --width W --height H] --feature NAME...
        --npy DIR | --hdr DIR | --png DIR
"""
import numpy as np

from .capi import PIXEL_FEATURES

f32 = np.float32
MISS = 0xFFFFFFFF
# the float images of oracle_shading_data()'s 17 floats: position 0:3, normal 3:6, outgoing 6:9, lambert_outgoing 9,
# diffuse_albedo 10:13, fresnel_0 13:16, roughness 16
FLOAT_FEATURES = ("position", "normal", "outgoing", "diffuse_albedo", "fresnel_0", "reprojection")


def world_to_projection_space(constants):
    """The (4, 4) float32 matrix of a constant buffer's byte image (per_frame_constants_t, offset 32)"""
    return np.frombuffer(np.ascontiguousarray(constants, np.uint8)[32:96].tobytes(), np.float32).reshape(4, 4).copy()


def camera_position(constants):
    return np.frombuffer(np.ascontiguousarray(constants, np.uint8)[144:156].tobytes(), np.float32).copy()


def distance(position, camera):
    """sqrt((d.x * d.x + d.y * d.y) + d.z * d.z), d = camera - position; position (..., 3)"""
    d = np.asarray(camera, f32) - np.asarray(position, f32)
    with np.errstate(all="ignore"):
        return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(f32)


def reprojection(position, matrix, width, height):
    """{X, Y, c_3, inside} of positions (..., 3) under the row-major world_to_projection_space `matrix` -> (..., 4) float32"""
    p, m = np.asarray(position, f32), np.asarray(matrix, f32).reshape(4, 4)
    with np.errstate(all="ignore"):
        c = [((m[i, 0] * p[..., 0] + m[i, 1] * p[..., 1]) + m[i, 2] * p[..., 2]) + m[i, 3] for i in (0, 1, 3)]
        w, h = f32(width), f32(height)
        x = (c[0] / c[2] + f32(1)) * (f32(0.5) * w) - f32(0.5)
        y = (c[1] / c[2] + f32(1)) * (f32(0.5) * h) - f32(0.5)
        inside = (c[2] > 0) & (x >= f32(-0.5)) & (x < w - f32(0.5)) & (y >= f32(-0.5)) & (y < h - f32(0.5))
    return np.stack([x, y, c[2], inside.astype(f32)], axis=-1).astype(f32)


def expected_images(shading_data, visibility, material_indices, constants, reprojection_matrix=None):
    """The seven images of a frame from its per-pixel oracle_shading_data() output: shading_data (height, width, 17)
    float32, visibility (height, width) uint32, material_indices (triangles,) uint8, constants: the frame's constant
    buffer.  -> {name: (height, width, 4)}; pixels with nothing visible hold zeros, the identity image
    {0xFFFFFFFF, 0xFFFFFFFF, x, y}."""
    s = np.ascontiguousarray(shading_data, f32)
    visibility = np.ascontiguousarray(visibility, np.uint32)
    height, width = visibility.shape
    covered = visibility != MISS
    if reprojection_matrix is None:
        reprojection_matrix = world_to_projection_space(constants)
    ones = np.ones((height, width), f32)
    images = {
        "position": np.dstack([s[..., 0:3], distance(s[..., 0:3], camera_position(constants))]),
        "normal": np.dstack([s[..., 3:6], s[..., 9]]),
        "outgoing": np.dstack([s[..., 6:9], ones]),
        "diffuse_albedo": np.dstack([s[..., 10:13], s[..., 16]]),
        "fresnel_0": np.dstack([s[..., 13:16], ones]),
        "reprojection": reprojection(s[..., 0:3], reprojection_matrix, width, height),
    }
    for name in images:
        # (as bits: a zeroed pixel is sixteen zero bytes, and no NaN of a covered pixel is touched)
        image = np.ascontiguousarray(images[name], f32).view(np.uint32)
        images[name] = np.where(covered[..., None], image, np.uint32(0)).astype(np.uint32).view(f32)
    materials = np.asarray(material_indices, np.uint8).astype(np.uint32)
    material = np.where(covered, materials[np.where(covered, visibility, 0)], np.uint32(MISS))
    ys, xs = np.mgrid[0:height, 0:width]
    images["identity"] = np.stack([visibility, material, xs, ys], axis=-1).astype(np.uint32)
    return images


# ---- previews ----------------------------------------------------------------------------------------------------

def u8(x):
    """The UNORM8 store: clamp to [0, 1], x * 255 + 0.5, truncate; a NaN gives 0"""
    x = np.asarray(x, f32)
    with np.errstate(all="ignore"):
        x = np.where(x > 0, np.minimum(x, f32(1)), f32(0)).astype(f32)
        return (x * f32(255) + f32(0.5)).astype(np.uint8)


def srgb8(x):
    """The sRGB8 code of encode_output(): u8(linear_to_srgb(clamp(x))) with the powf of csrc/glibc_math.h"""
    from .texture_conversion import powf
    x = np.asarray(x, f32)
    with np.errstate(all="ignore"):
        v = np.where(x > 0, np.minimum(x, f32(1)), f32(0)).astype(f32)
        s = np.where(v <= f32(0.0031308), f32(12.92) * v, f32(1.055) * powf(v, f32(1.0) / f32(2.4)).reshape(v.shape) - f32(0.055)).astype(f32)
    return u8(s)


def _rgba(r, g, b):
    return np.stack([r, g, b, np.full(r.shape, 255, np.uint8)], axis=-1).astype(np.uint8)


def check_range(range_low, range_high):
    if not (f32(range_high) > f32(range_low)):
        raise ValueError("the preview needs range_low < range_high")


def preview_direction(image):
    """normal, outgoing"""
    v = np.asarray(image, f32)
    return _rgba(*(u8(v[..., i] * f32(0.5) + f32(0.5)) for i in range(3)))


def preview_color(image):
    """diffuse_albedo, fresnel_0"""
    v = np.asarray(image, f32)
    return _rgba(*(srgb8(v[..., i]) for i in range(3)))


def preview_position(image, range_low, range_high):
    check_range(range_low, range_high)
    v, lo, hi = np.asarray(image, f32), f32(range_low), f32(range_high)
    with np.errstate(all="ignore"):
        grey = u8((v[..., 3] - lo) / (hi - lo))
    return _rgba(grey, grey, grey)


def preview_reprojection(image, range_low, range_high):
    check_range(range_low, range_high)
    v, hi = np.asarray(image, f32), f32(range_high)
    height, width = v.shape[:2]
    ys, xs = np.mgrid[0:height, 0:width]
    with np.errstate(all="ignore"):
        r = u8(((v[..., 0] - xs.astype(f32)) + hi) / (f32(2) * hi))
        g = u8(((v[..., 1] - ys.astype(f32)) + hi) / (f32(2) * hi))
    return _rgba(r, g, u8(v[..., 3]))


def preview_identity(image):
    primitive = np.asarray(image).view(np.uint32)[..., 0] if np.asarray(image).dtype != np.uint32 else np.asarray(image)[..., 0]
    h = (primitive.astype(np.uint64) * np.uint64(2654435761)).astype(np.uint32)
    h = np.where(primitive == MISS, np.uint32(0), h)
    return _rgba((h & 255).astype(np.uint8), ((h >> 8) & 255).astype(np.uint8), ((h >> 16) & 255).astype(np.uint8))


def preview(name, image, range=(0.0, 1.0)):
    """The bytes of encode_feature_preview() for the feature `name`: (height, width, 4) uint8"""
    if name in ("normal", "outgoing"):
        return preview_direction(image)
    if name in ("diffuse_albedo", "fresnel_0"):
        return preview_color(image)
    if name == "position":
        return preview_position(image, *range)
    if name == "reprojection":
        return preview_reprojection(image, *range)
    if name == "identity":
        return preview_identity(image)
    raise ValueError("%r is no feature (%s)" % (name, ", ".join(PIXEL_FEATURES)))


# ---- command line -------------------------------------------------------------------------------------------------

def main(arguments=None):
    import argparse
    import os

    from . import frame_images
    parser = argparse.ArgumentParser(prog="python -m vulkan_renderer_amd.feature_buffers", description="Writes feature images of a dataset's frame.")
    frame_images.add_dataset_arguments(parser, spp=False)
    parser.add_argument("--feature", action="append", choices=PIXEL_FEATURES, required=True)
    parser.add_argument("--range", type=float, nargs=2, default=None, metavar=("LOW", "HIGH"), help="of the position and reprojection previews (--png)")
    output = parser.add_mutually_exclusive_group(required=True)
    output.add_argument("--npy", metavar="DIR")
    output.add_argument("--hdr", metavar="DIR", help="Radiance files of the float images, through the device's encoder")
    output.add_argument("--png", metavar="DIR", help="PNG files of the previews, through the device's encoder")
    options = parser.parse_args(arguments)
    directory = options.npy or options.hdr or options.png
    os.makedirs(directory, exist_ok=True)
    with frame_images.open_dataset(options) as scene:
        scene.render_visibility()
        images = scene.render_features(options.feature)
        for name, image in images.items():
            if options.npy:
                np.save(os.path.join(directory, name + ".npy"), image)
            elif options.hdr:
                if name == "identity":
                    raise SystemExit("the identity image holds integers: write it with --npy or --png")
                with open(os.path.join(directory, name + ".hdr"), "wb") as file:
                    file.write(scene.encode_hdr(image))
            else:
                value_range = options.range
                if value_range is None:
                    # (position: up to the farthest covered pixel; reprojection: sixteen pixels of motion saturate)
                    value_range = (0.0, float(image[..., 3].max()) or 1.0) if name == "position" else (0.0, 16.0)
                with open(os.path.join(directory, name + ".png"), "wb") as file:
                    file.write(scene.encode_png(scene.feature_preview(name, image, value_range)))
            print("%s -> %s" % (name, directory))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
