"""Frames and expectations shared by tests/test_feature_buffers.py (CPU: the numpy rules and the conditions on the frames)
and tests/test_gpu_feature_buffers.py (the kernels against the oracle).  Not collected by pytest.

The frames: the session dataset under a camera 5 mm above the ground plane that looks along it - the horizon cuts the frame,
so a good part of the pixels sees nothing, and the far ground is seen at less than 2e-3 from edge-on, which runs the
normal-offset branch of get_shading_data() - at 83x45 (partial blocks on both edges), 16x16 (one block) and 7x3 (less than a
wave); and a textured dataset under a grazing camera, where the sampler takes several tap counts."""
import ctypes as C
import functools
import math

import numpy as np

import oracle
from vulkan_renderer_amd import feature_buffers, renderer, synthetic

CONFIG = 3
EXTENTS = [(83, 45), (16, 16), (7, 3)]
CAMERA = dict(position=(-3.0, -2.0, 0.005), rotation_x=0.5 * math.pi - 0.0008, rotation_z=1.3 * math.pi)
# the camera of the reprojection matrix: moved into the scene and turned, so that covered pixels of the first camera lie
# behind it (c_3 <= 0) and others beside its frame
SECOND_CAMERA = dict(position=(0.5, 1.0, 0.6), rotation_x=0.45 * math.pi, rotation_z=1.05 * math.pi)
TEXTURED_DATASET = dict(grid=64, box_count=24, seed=1234, ltc_resolution=16, fresnel_count=8, textured=True, texture_size=64)
TEXTURED_CAMERA = dict(position=(-3.0, -2.0, 0.12), rotation_x=0.49 * math.pi, rotation_z=1.3 * math.pi)
FLOAT_NAMES = ("position", "normal", "outgoing", "diffuse_albedo", "fresnel_0", "reprojection")


def set_camera(scene, camera):
    default = synthetic.DEFAULT_CAMERA
    scene.set_camera(camera["position"], camera["rotation_x"], camera["rotation_z"], default["vertical_fov"], default["near"], default["far"])


def apply_frame(scene, dataset, width, height, camera=CAMERA, **overrides):
    """BASELINE config 3 at the extent and under the camera of a test frame; a HostScene gets no acceleration structure
    (and no shadow rays, which the shading data do not depend on)"""
    if not scene._device:
        overrides = dict(overrides, trace_shadow_rays=False, acceleration_structure=False)
    else:
        overrides = dict(overrides, acceleration_structure=True)
    renderer.setup_config(scene, CONFIG, dataset, width, height, **overrides)
    set_camera(scene, camera)


def second_matrix(scene):
    """world_to_projection_space of SECOND_CAMERA at the scene's extent; the scene's own camera is put back"""
    camera = scene.app.scene_specification.camera
    kept = (tuple(camera.position_world_space), camera.rotation_x, camera.rotation_z)
    set_camera(scene, SECOND_CAMERA)
    matrix = feature_buffers.world_to_projection_space(scene.constants())
    camera.position_world_space[:] = kept[0]
    camera.rotation_x, camera.rotation_z = kept[1], kept[2]
    return matrix


def oracle_frame(scene, visibility=None):
    """-> (oracle frame, inputs) of a HostScene / Renderer; visibility: the device's, or None for the oracle's own"""
    inputs = scene.host_inputs()
    bvh = oracle.Bvh(inputs["quantized_positions"], inputs["dequantization_factor"], inputs["dequantization_summand"])
    if visibility is None:
        e, camera = scene.app.swapchain.extent, scene.app.scene_specification.camera
        visibility = oracle.primary_visibility(inputs["constants"], bvh, e.width, e.height, camera.near, camera.far)
    inputs["visibility"] = np.ascontiguousarray(visibility, np.uint32)
    return oracle.make_frame(inputs, scene.oracle_settings(), bvh), inputs


def shading_data(frame, math_mode=0):
    """oracle_shading_data() of every pixel: (height, width, 17) float32, in the given math mode (restored)"""
    out = np.zeros((frame.height, frame.width, 17), np.float32)
    pointer = C.POINTER(C.c_float)
    call = oracle.lib().oracle_shading_data
    oracle.set_math_mode(math_mode)
    try:
        for y in range(frame.height):
            for x in range(frame.width):
                call(C.byref(frame), x, y, out[y, x].ctypes.data_as(pointer))
    finally:
        oracle.set_math_mode(0)
    return out


def expected(scene, visibility=None, math_mode=0, reprojection_matrix=None):
    """-> (the seven images by the oracle and the numpy rules, the oracle's shading data, inputs, frame)"""
    frame, inputs = oracle_frame(scene, visibility)
    data = shading_data(frame, math_mode)
    images = feature_buffers.expected_images(data, inputs["visibility"], inputs["material_indices"], inputs["constants"], reprojection_matrix)
    return images, data, inputs, frame


def assert_frame_conditions(images, data, inputs, extent, second=None):
    """What the frames are chosen for, on the oracle's side"""
    visibility = inputs["visibility"]
    covered = visibility != 0xFFFFFFFF
    assert covered.any()
    if extent != (7, 3):
        assert 0.05 <= 1.0 - covered.mean() <= 0.95, covered.mean()
    if extent == (83, 45):
        # the normal-offset branch: max(0, 1e-3 - n.o) > 0 leaves lambert_outgoing below 2e-3
        assert (data[..., 9][covered] < 2.0e-3).any(), data[..., 9][covered].min()
    if second is not None and extent != (7, 3):
        reprojected = feature_buffers.reprojection(data[..., 0:3], second, extent[0], extent[1])[covered]
        assert (reprojected[:, 2] <= 0).any() and ((reprojected[:, 2] > 0) & (reprojected[:, 3] == 0)).any() and (reprojected[:, 3] == 1).any()


def tap_counts(frame, inputs):
    """The distinct tap counts of the texture reads of a textured frame, by oracle_texture_footprint_batch"""
    sampler_inputs = oracle.texture_sampler_inputs(frame).reshape(-1, 6)
    sampler_inputs = sampler_inputs[~np.isnan(sampler_inputs[:, 0])]
    texture = next(t for t in inputs["material_textures"] if t["width"])
    return set(oracle.texture_footprint_batch(texture, sampler_inputs)[:, 0].tolist())


@functools.lru_cache(maxsize=None)
def code_starts():
    status, starts = oracle.srgb8_code_starts()
    assert status == 0
    return starts
