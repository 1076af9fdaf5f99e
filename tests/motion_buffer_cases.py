"""Inputs and expectations shared by tests/test_motion_buffers.py (CPU: the numpy restatement against the oracle and against
binary64, and the conditions on the cases) and tests/test_gpu_motion_buffers.py (the kernel against the restatement).  Not
collected by pytest.

The frames are those of tests/feature_buffer_cases.py: the session dataset under the camera 5 mm above the ground at 83x45,
16x16 and 7x3.  The mesh on the device is the dataset's; what varies is the array of PREVIOUS positions, a displaced copy of
the mesh in codes:
    rigid          every vertex by the same RIGID_SHIFT codes
    per_triangle   every triangle as a whole by up to 2000 codes per axis, as test_images_follow_update_geometry moves them
    large          every triangle as a whole by up to LARGE_SHIFT codes per axis (several metres): previous positions out
                   of the frame on every side and behind the camera, under the frame's own matrix
    still          no shift
A shift that would leave the 21 bits of a code is clipped (the ground spans the de-quantisation box): displaced() says which
triangles kept their shape.  The small shifts are seen under the second camera of the feature buffer tests, under which the
current positions already fall into every class."""
import numpy as np

import feature_buffer_cases as frames
from vulkan_renderer_amd import feature_buffers, motion_buffers, scene_update

f32 = np.float32
EXTENTS = frames.EXTENTS
MESHES = ("rigid", "per_triangle", "large", "still")
# 1.4 cm, 0.9 cm and 1.1 cm: the box is 20 m wide, a little more than 1 m high and 2^21 codes across either way
RIGID_SHIFT = np.array([1500, -900, 20000], np.int64)
LARGE_SHIFT = 600000
CLASSES = ("inside", "outside_x", "outside_y", "behind")


def displaced(words, name):
    """-> (the previous position words (3 T, 2) uint32 of mesh `name`, exact (T,) bool: the triangles that no clipping bent)"""
    codes = scene_update.unpack_positions(words).astype(np.int64).reshape(-1, 3, 3)
    rng = np.random.default_rng(33)
    if name == "still":
        shift = np.zeros(3, np.int64)
    elif name == "rigid":
        shift = RIGID_SHIFT
    else:
        reach = 2000 if name == "per_triangle" else LARGE_SHIFT
        shift = rng.integers(-reach, reach + 1, (len(codes), 1, 3))
    moved = codes + shift
    clipped = np.clip(moved, 0, scene_update.CODE_MAX)
    return scene_update.pack_positions(clipped.astype(np.uint32).reshape(-1, 3)), (moved == clipped).all(axis=(1, 2))


def previous_matrix(scene, name):
    """The matrix that mesh `name` is seen under: the frame's own for the large shifts, the second camera's otherwise"""
    if name == "large":
        return feature_buffers.world_to_projection_space(scene.constants())
    return frames.second_matrix(scene)


def classes(reprojection, covered, width, height):
    """-> {class: number of covered pixels}: where the previous position lies under the previous matrix"""
    x, y, w = (reprojection[..., i][covered] for i in range(3))
    with np.errstate(all="ignore"):
        in_x, in_y = (x >= -0.5) & (x < width - 0.5), (y >= -0.5) & (y < height - 0.5)
    front = w > 0
    return {"inside": int((reprojection[..., 3][covered] == 1).sum()), "outside_x": int((front & ~in_x).sum()),
            "outside_y": int((front & ~in_y).sum()), "behind": int((w <= 0).sum())}


def expected(scene, visibility, name):
    """-> (images of the numpy restatement, counts, previous words, matrix) for a HostScene or Renderer that
    frames.apply_frame() set up, the visibility of its frame and mesh `name`"""
    inputs = scene.host_inputs()
    previous, _ = displaced(inputs["quantized_positions"], name)
    matrix = previous_matrix(scene, name)
    counts = {}
    images = motion_buffers.expected_images(visibility, inputs["quantized_positions"], previous, inputs["constants"], matrix, counts)
    for image in images.values():
        image.setflags(write=False)
    return images, counts, previous, matrix


def assert_conditions(results):
    """What the meshes are there for, on the numpy side.  results: {(name, extent): (images, counts, visibility)} over MESHES
    and EXTENTS"""
    for name in MESHES:
        totals = dict.fromkeys(CLASSES, 0)
        for extent in EXTENTS:
            images, counts, visibility = results[(name, extent)]
            covered = visibility != 0xFFFFFFFF
            found = classes(images["reprojection"], covered, *extent)
            assert counts["covered"] == int(covered.sum()) > 0 and counts["inside"] == found["inside"]
            for image in images.values():
                assert not image[~covered].view(np.uint32).any()
            assert (images["previous_position"][covered][:, 3] == 1).all()
            assert images["motion"][..., 3].tobytes() == images["reprojection"][..., 3].tobytes()
            if name == "still":
                # nothing moved: |Q - P| is 0, not merely small
                assert counts["moved"] == 0 and not images["motion"][..., 2].any()
            else:
                assert counts["moved"] > 0.9 * counts["covered"]
            if extent == (83, 45):
                assert all(found[key] > 0 for key in CLASSES), (name, found)
            for key in CLASSES:
                totals[key] += found[key]
        assert all(totals[key] > 0 for key in CLASSES), (name, totals)
