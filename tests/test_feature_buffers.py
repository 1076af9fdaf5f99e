"""Feature buffers (include/vkr_feature_buffers.h) without a GPU: the numpy restatements of the derived values and of the
previews (vulkan_renderer_amd/feature_buffers.py) against independent statements, the convention of the reprojection on
CPU-shaded test frames, the conditions that the frames of tests/test_gpu_feature_buffers.py are chosen for, and the ctypes
mirror."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import feature_buffer_cases as cases
from vulkan_renderer_amd import capi, feature_buffers, renderer, synthetic

f32 = np.float32
U = 2.0 ** -24  # unit roundoff of binary32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Largest |X - x|, |Y - y| of a covered pixel reprojected with its own frame's matrix, measured on the CPU over the four test
# frames below (83x45 4.32e-3, 16x16 7.5e-4, 7x3 3.0e-4, textured 83x45 4.11e-3 pixel): the float32 position of a point
# 5 - 15 m away, seen from 5 mm above the plane it lies in.  The test allows four times as much.
MEASURED_REPROJECTION_DEVIATION = 4.4e-3


def around(values, steps=4):
    """every value and the `steps` floats below and above it (x * 255 + 0.5 rounds twice: the float at which a code begins
    lies a few floats beside the real number (c - 0.5) / 255)"""
    values = np.asarray(values, f32)
    out, below, above = [values], values, values
    for _ in range(steps):
        below, above = np.nextafter(below, f32(-np.inf)), np.nextafter(above, f32(np.inf))
        out += [below, above]
    return np.concatenate(out)


SPECIAL = np.array([0.0, -0.0, 1.0, -1.0, 0.5, 1.0e-45, -1.0e-45, 1.0e-30, 3.0e38, -3.0e38, np.inf, -np.inf, np.nan], f32)


# ---- the derived values --------------------------------------------------------------------------------------------

def test_distance_equals_binary64_within_its_roundings():
    """d_i = c_i - p_i is rounded once (relative U); d_i^2 then carries 3 U, each of the two additions adds U to a sum of
    positive terms (5 U), the root halves that and rounds once more: 3.5 U relative, asserted as 4 U.  Zero, infinity and
    NaN come out as binary64 has them."""
    rng = np.random.default_rng(5)
    position = (rng.normal(size=(20000, 3)) * 10.0 ** rng.uniform(-3, 3, (20000, 1))).astype(f32)
    camera = (rng.normal(size=3) * 3.0).astype(f32)
    got = feature_buffers.distance(position, camera).astype(np.float64)
    true = np.sqrt(((camera.astype(np.float64) - position.astype(np.float64)) ** 2).sum(axis=1))
    assert (np.abs(got - true) <= 4.0 * U * true).all(), np.abs(got / true - 1.0).max() / U
    assert feature_buffers.distance(camera[None], camera)[0] == 0.0
    special = feature_buffers.distance(np.array([[np.inf, 0, 0], [np.nan, 0, 0], [0, -np.inf, 1]], f32), np.zeros(3, f32))
    assert np.isinf(special[0]) and np.isnan(special[1]) and np.isinf(special[2])


def test_reprojection_equals_binary64_within_its_roundings():
    """c_i: four products and three additions; with S_i the sum of the absolute values of its four terms,
    |dc_i| <= 4 U S_i (each product U of itself, each addition U of a partial sum that S_i bounds).  q = c_0 / c_3:
    |dq| <= (dc_0 + |q| dc_3) / |c_3| + U |q|.  X = (q + 1) (w / 2) - 1 / 2: the addition U |q + 1|, the product U more of
    the same (w / 2 is exact), the subtraction U |X|: |dX| <= (w / 2) (dq + 2 U |q + 1|) + U |X|.  First order in U; the
    test allows 1 % more for the rest.  inside is the rule applied to the float32 X, Y and c_3 themselves."""
    rng = np.random.default_rng(6)
    n, width, height = 20000, 83, 45
    position = (rng.normal(size=(n, 3)) * 5.0).astype(f32)
    matrix = rng.normal(size=(4, 4)).astype(f32)
    got = feature_buffers.reprojection(position, matrix, width, height)
    p, m = position.astype(np.float64), matrix.astype(np.float64)
    terms = [np.stack([m[i, 0] * p[:, 0], m[i, 1] * p[:, 1], m[i, 2] * p[:, 2], np.full(n, m[i, 3])], axis=1) for i in (0, 1, 3)]
    c = [t.sum(axis=1) for t in terms]
    dc = [4.0 * U * np.abs(t).sum(axis=1) for t in terms]
    for axis, extent in ((0, width), (1, height)):
        q = c[axis] / c[2]
        dq = (dc[axis] + np.abs(q) * dc[2]) / np.abs(c[2]) + U * np.abs(q)
        exact = (q + 1.0) * (0.5 * extent) - 0.5
        bound = 1.01 * (0.5 * extent * (dq + 2.0 * U * np.abs(q + 1.0)) + U * np.abs(exact))
        assert (np.abs(got[:, axis] - exact) <= bound).all(), (np.abs(got[:, axis] - exact) / bound).max()
    assert (np.abs(got[:, 2] - c[2]) <= 1.01 * dc[2]).all()
    x, y, w = got[:, 0], got[:, 1], got[:, 2]
    inside = (w > 0) & (x >= -0.5) & (x < width - 0.5) & (y >= -0.5) & (y < height - 0.5)
    assert np.array_equal(got[:, 3], inside.astype(f32)) and 0 < inside.sum() < n and (w <= 0).any()


def test_reprojection_of_special_values():
    """c_3 <= 0, zero, infinity and NaN: inside is 0 whenever a comparison has a NaN or c_3 is not positive"""
    identity = np.eye(4, dtype=f32)
    # (with the identity c_3 = 1: make w the z coordinate instead)
    matrix = identity.copy()
    matrix[3] = (0, 0, 1, 0)
    position = np.array([[0, 0, 1], [0, 0, -1], [0, 0, 0], [1, 1, 0], [np.nan, 0, 1], [0, np.inf, 1], [0, 0, np.inf], [0.999, -0.999, 1], [1.001, 0, 1]], f32)
    got = feature_buffers.reprojection(position, matrix, 8, 4)
    assert got[:, 3].tolist() == [1, 0, 0, 0, 0, 0, 0, 1, 0]
    assert got[0, :3].tolist() == [3.5, 1.5, 1.0]
    assert got[1, 2] == -1.0 and np.isnan(got[2, 0]) and np.isinf(got[3, 0]) and np.isnan(got[4, 0]) and np.isnan(got[5, 1]) and np.isnan(got[6, 0])


# ---- the previews --------------------------------------------------------------------------------------------------

def scalar_u8(x):
    """clamp to [0, 1], x * 255 + 0.5, truncate; NaN -> 0: one float32 operation at a time"""
    x = f32(x)
    if x != x:
        return 0
    x = min(max(x, f32(0)), f32(1))
    return int(f32(f32(x * f32(255)) + f32(0.5)))


def test_u8_at_every_code_boundary():
    boundaries = np.array([(c - 0.5) / 255.0 for c in range(1, 256)], np.float64).astype(f32)
    values = np.concatenate([around(boundaries), around(np.array([0.0, 1.0], f32)), SPECIAL])
    got = feature_buffers.u8(values)
    assert got.tolist() == [scalar_u8(v) for v in values]
    assert set(got.tolist()) == set(range(256))
    # each boundary separates its two codes within the floats next to it, and the code never decreases
    for c, b in enumerate(boundaries, start=1):
        codes = [scalar_u8(v) for v in np.sort(around(np.array([b], f32)))]
        assert set(codes) == {c - 1, c} and codes == sorted(codes), (c, codes)


def test_color_preview_at_every_code_start():
    starts = cases.code_starts().view(f32)
    below = np.nextafter(starts[1:], f32(-np.inf))
    assert feature_buffers.srgb8(starts).tolist() == list(range(256))
    assert feature_buffers.srgb8(below).tolist() == list(range(255))
    from helpers import srgb8_by_starts
    values = np.concatenate([around(starts), SPECIAL, np.linspace(-0.5, 1.5, 4001).astype(f32)])
    assert np.array_equal(feature_buffers.srgb8(values), srgb8_by_starts(values, cases.code_starts()))
    image = np.zeros((2, 3, 4), f32)
    image[..., 0], image[..., 1], image[..., 2], image[..., 3] = starts[7], below[99], 2.0, np.nan
    assert np.array_equal(feature_buffers.preview("diffuse_albedo", image), np.broadcast_to(np.array([7, 99, 255, 255], np.uint8), (2, 3, 4)))
    assert np.array_equal(feature_buffers.preview("fresnel_0", image), feature_buffers.preview("diffuse_albedo", image))


def test_direction_preview():
    # v * 0.5 + 0.5 crosses a code boundary where v = (2 c - 1) / 255 - 1
    values = np.concatenate([around(np.array([(2.0 * c - 1.0) / 255.0 - 1.0 for c in range(1, 256)], np.float64).astype(f32)), SPECIAL])
    image = np.zeros((1, len(values), 4), f32)
    image[0, :, 0], image[0, :, 1], image[0, :, 2] = values, values[::-1], -values
    expected = [[scalar_u8(f32(f32(v * f32(0.5)) + f32(0.5))) for v in row] for row in (values, values[::-1], -values)]
    for name in ("normal", "outgoing"):
        got = feature_buffers.preview(name, image)
        assert got[0, :, :3].T.tolist() == expected and (got[..., 3] == 255).all()


def test_position_preview_and_its_range():
    low, high = f32(0.25), f32(7.5)
    boundaries = np.array([low + (high - low) * (c - 0.5) / 255.0 for c in range(1, 256)], np.float64).astype(f32)
    values = np.concatenate([around(boundaries), around(np.array([low, high])), SPECIAL])
    image = np.zeros((1, len(values), 4), f32)
    image[0, :, 3] = values
    got = feature_buffers.preview("position", image, (low, high))
    with np.errstate(all="ignore"):
        expected = [scalar_u8(f32(f32(v - low) / f32(high - low))) for v in values]
    assert got[0, :, 0].tolist() == expected and np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2])
    assert len(set(expected)) == 256 and (got[..., 3] == 255).all()
    for bad in ((1.0, 1.0), (2.0, 1.0), (np.nan, 1.0), (0.0, np.nan)):
        with pytest.raises(ValueError):
            feature_buffers.preview("position", image, bad)
        with pytest.raises(ValueError):
            feature_buffers.preview("reprojection", image, bad)


def test_reprojection_preview():
    high = f32(4.0)
    rng = np.random.default_rng(8)
    image = np.zeros((5, 9, 4), f32)
    image[..., 0] = (np.arange(9)[None, :] + rng.uniform(-6, 6, (5, 9))).astype(f32)
    image[..., 1] = (np.arange(5)[:, None] + rng.uniform(-6, 6, (5, 9))).astype(f32)
    image[..., 3] = rng.integers(0, 2, (5, 9))
    image[0, 0, 0], image[0, 1, 1], image[0, 2, 3] = np.nan, np.inf, np.nan
    got = feature_buffers.preview("reprojection", image, (0.0, high))
    with np.errstate(all="ignore"):
        for y in range(5):
            for x in range(9):
                red = scalar_u8(f32(f32(f32(image[y, x, 0] - f32(x)) + high) / f32(f32(2) * high)))
                green = scalar_u8(f32(f32(f32(image[y, x, 1] - f32(y)) + high) / f32(f32(2) * high)))
                assert got[y, x].tolist() == [red, green, scalar_u8(image[y, x, 3]), 255], (x, y)
    # no motion is the middle grey, a motion of +-range_high saturates
    still = np.zeros((1, 3, 4), f32)
    still[0, :, 0] = [0.0, 1.0 + 4.0, 2.0 - 4.0]
    assert feature_buffers.preview("reprojection", still, (0.0, high))[0, :, 0].tolist() == [128, 255, 0]


def test_identity_preview():
    primitives = np.array([0, 1, 2, 255, 256, 65535, 8479, 0x7FFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF], np.uint32)
    image = np.zeros((1, len(primitives), 4), np.uint32)
    image[0, :, 0] = primitives
    image[0, :, 1:] = 0xABCD
    got = feature_buffers.preview("identity", image)
    for i, primitive in enumerate(int(p) for p in primitives):
        h = (primitive * 2654435761) % (1 << 32) if primitive != 0xFFFFFFFF else 0
        assert got[0, i].tolist() == [h & 255, (h >> 8) & 255, (h >> 16) & 255, 255]
    assert got[0, -1].tolist() == [0, 0, 0, 255]
    with pytest.raises(ValueError):
        feature_buffers.preview("depth", image)


# ---- the frames ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def textured_dataset(tmp_path_factory):
    return synthetic.write_dataset(str(tmp_path_factory.mktemp("feature_textured")), **cases.TEXTURED_DATASET)


@pytest.fixture(scope="module")
def cpu_frames(dataset, textured_dataset):
    """[(extent, images by the oracle with the second camera's reprojection, shading data, inputs, frame, textured)]"""
    frames = []
    for extent, source, camera in [(e, dataset, cases.CAMERA) for e in cases.EXTENTS] + [((83, 45), textured_dataset, cases.TEXTURED_CAMERA)]:
        scene = renderer.HostScene()
        try:
            cases.apply_frame(scene, source, extent[0], extent[1], camera)
            second = cases.second_matrix(scene)
            frames.append((extent,) + cases.expected(scene, reprojection_matrix=second) + (source is textured_dataset, second))
        finally:
            scene.close()
    return frames


def test_frames_meet_their_conditions(cpu_frames):
    for extent, images, data, inputs, frame, textured, second in cpu_frames:
        if textured:
            assert len(cases.tap_counts(frame, inputs)) >= 3
            cases.assert_frame_conditions(images, data, inputs, (0, 0))
        else:
            cases.assert_frame_conditions(images, data, inputs, extent, second)
        covered = inputs["visibility"] != 0xFFFFFFFF
        for name in cases.FLOAT_NAMES:
            assert not images[name][~covered].view(np.uint32).any(), name
        identity = images["identity"]
        assert (identity[~covered][:, :2] == 0xFFFFFFFF).all() and (identity[covered][:, 1] < 256).all()
        assert np.array_equal(identity[..., 2], np.broadcast_to(np.arange(extent[0]), identity.shape[:2]))
        assert np.array_equal(identity[..., 3], np.broadcast_to(np.arange(extent[1])[:, None], identity.shape[:2]))
        assert (images["outgoing"][covered][:, 3] == 1).all() and (images["position"][covered][:, 3] > 0).all()


def test_reprojection_with_the_frames_own_matrix_returns_the_pixel(cpu_frames):
    """The convention: world_to_projection_space of the frame itself sends the shading point of pixel (x, y) to (x, y).  A
    flipped axis or a shift by half a pixel misses by 0.5 pixel or more; the bound is far below that."""
    bound = 4.0 * MEASURED_REPROJECTION_DEVIATION
    assert bound < 0.25
    largest = 0.0
    for extent, images, data, inputs, frame, textured, second in cpu_frames:
        covered = inputs["visibility"] != 0xFFFFFFFF
        own = feature_buffers.reprojection(data[..., 0:3], feature_buffers.world_to_projection_space(inputs["constants"]), extent[0], extent[1])
        ys, xs = np.mgrid[0:extent[1], 0:extent[0]]
        deviation = np.maximum(np.abs(own[..., 0] - xs), np.abs(own[..., 1] - ys))[covered]
        print(extent, "textured" if textured else "", "largest deviation %.3e pixel" % deviation.max())
        largest = max(largest, float(deviation.max()))
        assert (deviation <= bound).all() and (own[..., 3][covered] == 1).all() and (own[..., 2][covered] > 0).all()
    # the recorded measurement is the one these frames give (it is what the bound comes from)
    assert 0.5 * MEASURED_REPROJECTION_DEVIATION <= largest <= MEASURED_REPROJECTION_DEVIATION


# ---- the binding ---------------------------------------------------------------------------------------------------

def test_ctypes_mirror():
    header = open(os.path.join(ROOT, "include", "vkr_feature_buffers.h")).read()
    enum = re.search(r"typedef enum pixel_feature_e \{(.*?)\} pixel_feature_t;", header, re.S).group(1)
    names = re.findall(r"^\s*pixel_feature_(\w+)", enum, re.M)
    assert names[-1] == "count" and tuple(names[:-1]) == capi.PIXEL_FEATURES
    assert C.sizeof(capi.FeatureBuffers) == len(capi.PIXEL_FEATURES) * 8 + 64
    assert capi.FeatureBuffers.reprojection_matrix.offset == len(capi.PIXEL_FEATURES) * 8
    lib = capi.load()
    for symbol in ("render_feature_buffers", "encode_feature_preview"):
        assert "VKR_API int %s(" % symbol in header
        assert hasattr(lib, symbol) and symbol in capi.SIGNATURES
