"""Meshes and motions of the scene update tests (include/vkr_scene_update.h), and the helper that rewrites the position
block of a .vks file.

The meshes are the smallest that reach every branch of csrc/bvh_refit.hip: those of test_gpu_bvh_small_meshes.py with
1, 2, 3 and 17 triangles (a single leaf with no inner node and no wide tree, level loops that run once, a collapse with
more than one level), one of a few hundred triangles with long thin diagonal slats, which the device SAH builder splits
into fragments, and one with an occluder under the first light of config 3.

Every mesh has a floor that spans its box and stays, so that the de-quantisation box of the file - the tight box of the
mesh - holds every moved vertex: quantized() asserts that no vertex was clamped."""
import struct

import numpy as np

from test_gpu_bvh_small_meshes import FLOOR_QUAD, MESHES as SMALL_MESHES
from vulkan_renderer_amd import scene_update, synthetic

BUILDERS = ("sah_device", "lbvh_device", "sah_host")
WIDTH, HEIGHT = 64, 36


def slat_mesh(slats=150, others=100, seed=23):
    """the floor, `slats` slivers 2 to 3 m long and 5 to 60 cm wide that run diagonally through their boxes, and `others`
    small triangles between them"""
    rng = np.random.default_rng(seed)
    centres = np.stack([rng.uniform(-3.5, 3.5, slats), rng.uniform(-2.0, 5.0, slats), rng.uniform(0.8, 1.8, slats)], -1)
    along = np.stack([rng.choice([-1.0, 1.0], slats), rng.choice([-1.0, 1.0], slats), rng.uniform(-0.3, 0.3, slats)], -1)
    along /= np.linalg.norm(along, axis=-1, keepdims=True)
    across = np.cross(along, [0.0, 0.0, 1.0])
    across /= np.linalg.norm(across, axis=-1, keepdims=True)
    length, width = rng.uniform(2.0, 3.0, slats)[:, None], rng.uniform(0.05, 0.6, slats)[:, None]
    slivers = np.stack([centres - 0.5 * length * along, centres + 0.5 * length * along, centres + width * across], 1)
    small = np.stack([rng.uniform(-3.0, 3.0, others), rng.uniform(-1.0, 5.0, others), rng.uniform(0.4, 1.8, others)], -1)[:, None, :] + rng.uniform(-0.2, 0.2, (others, 3, 3))
    return np.concatenate([np.array(FLOOR_QUAD, np.float64), slivers, small], 0)


# a quad of 2 m x 2 m under the first light of config 3 ((-1.5, 1.5, 2.2), facing down), and a ceiling triangle that keeps
# the box of the mesh as high as the occluder ever gets
OCCLUDER = [[[-2.5, 0.5, 1.2], [-0.5, 0.5, 1.2], [-0.5, 2.5, 1.2]], [[-2.5, 0.5, 1.2], [-0.5, 2.5, 1.2], [-2.5, 2.5, 1.2]]]
CEILING = [[[7.0, 7.0, 2.0], [8.0, 7.0, 2.0], [7.0, 8.0, 2.0]]]

MESHES = dict(SMALL_MESHES)
MESHES["slats"] = slat_mesh()
MESHES["occluder"] = np.array(FLOOR_QUAD + OCCLUDER + CEILING, np.float64)
# triangles that never move
FIXED = {1: 0, 2: 1, 3: 2, 17: 2, "slats": 2, "occluder": 2}


def rotate_about_z(triangles, angle):
    """every triangle turned about the vertical through its centroid"""
    centre = triangles.mean(axis=1, keepdims=True)
    c, s = np.cos(angle), np.sin(angle)
    d = triangles - centre
    return centre + np.stack([c * d[..., 0] - s * d[..., 1], s * d[..., 0] + c * d[..., 1], d[..., 2]], -1)


def motion(name, step):
    """-> the positions (T, 3, 3) float64 of mesh `name` at step 1, 2, ... of its motion (step 0: at rest)"""
    rest = MESHES[name]
    if step == 0:
        return rest.copy()
    moved = rest.copy()
    if name == 1:
        # the only triangle shrinks towards its centroid: inside its own box
        centre = rest.mean(axis=1, keepdims=True)
        return centre + (rest - centre) * (1.0 - 0.1 * min(step, 5))
    if name == 2:
        # the second half of the floor shrinks; the first one keeps the box
        centre = rest[1:].mean(axis=1, keepdims=True)
        moved[1:] = centre + (rest[1:] - centre) * (1.0 - 0.1 * min(step, 5))
        return moved
    if name == 3:
        # the triangle above the floor comes down and drifts (the box of the mesh ends at its rest height)
        moved[2] += np.array([0.4, 0.3, -0.15]) * min(step, 5)
        return moved
    if name == "occluder":
        # out of the shaft of the first light, towards the second
        moved[2:4] += np.array([2.6, 0.0, 0.3]) * (step % 2)
        return moved
    fixed = np.arange(len(rest)) < FIXED[name]
    if name == "slats":
        # the slats turn as well, so that the longest axis of their boxes changes
        moved[2:152] = rotate_about_z(rest[2:152], 0.4 * step)
    return scene_update.wobble(moved, 0.9 * step, 0.3, fixed=fixed)


def write_case(directory, name):
    """-> the dataset dict of mesh `name` at rest, its scene written like test_gpu_bvh_small_meshes.py does"""
    positions = MESHES[name]
    dataset = synthetic.write_dataset(str(directory), grid=8, box_count=0, ltc_resolution=16, fresnel_count=8)
    normals = np.cross(positions[:, 1] - positions[:, 0], positions[:, 2] - positions[:, 0])
    normals /= np.linalg.norm(normals, axis=-1, keepdims=True)
    names = synthetic.write_material_textures(dataset["textures"])
    # (unsorted: triangle t of the file is triangle t of MESHES)
    synthetic.write_vks(dataset["scene"], positions, np.repeat(normals[:, None, :], 3, 1), positions[:, :, :2] * 0.5, np.zeros(len(positions), np.uint8), names, sort_triangles=False)
    return dataset


def read_vks_header(path):
    """-> (triangle_count, factor, summand, offset of the position block)"""
    with open(path, "rb") as f:
        data = f.read()
    magic, version, material_count, triangle_count = struct.unpack_from("<IIQQ", data, 0)
    assert magic == 0x00ABCABC and version == 1
    factor, summand = np.array(struct.unpack_from("<fff", data, 24), np.float32), np.array(struct.unpack_from("<fff", data, 36), np.float32)
    offset = 48
    for _ in range(material_count):
        length, = struct.unpack_from("<Q", data, offset)
        offset += 8 + length + 1
    return int(triangle_count), factor, summand, offset


def read_vks_positions(path):
    """-> the position words (3 T, 2) uint32 of a scene file"""
    triangle_count, _, _, offset = read_vks_header(path)
    with open(path, "rb") as f:
        f.seek(offset)
        return np.frombuffer(f.read(24 * triangle_count), np.uint32).reshape(-1, 2).copy()


def rewrite_vks_positions(source, target, words):
    """copies scene file `source` to `target` with its position block replaced by `words` (3 T, 2) uint32"""
    triangle_count, _, _, offset = read_vks_header(source)
    words = np.ascontiguousarray(words, np.uint32)
    assert words.shape == (3 * triangle_count, 2)
    with open(source, "rb") as f:
        data = bytearray(f.read())
    data[offset:offset + words.nbytes] = words.tobytes()
    with open(target, "wb") as f:
        f.write(bytes(data))


def quantized(dataset, positions):
    """-> the position words of `positions` in the de-quantisation box of the dataset's scene; no vertex may leave that box"""
    _, factor, summand, _ = read_vks_header(dataset["scene"])
    codes, clamped = scene_update.quantize(positions, factor, summand)
    assert not clamped.any(), "%d vertices left the de-quantisation box" % int(clamped.sum())
    return scene_update.pack_positions(codes)
