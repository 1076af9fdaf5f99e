"""Motion buffers (include/vkr_motion_buffers.h) without a GPU: the numpy restatement (vulkan_renderer_amd/motion_buffers.py)
against the CPU oracle's shading point, against the feature buffers' reprojection and against binary64, the conditions that
the meshes of tests/motion_buffer_cases.py are chosen for, the ctypes mirror and the refusals that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import feature_buffer_cases as frames
import motion_buffer_cases as cases
from helpers import flush_c_output
from vulkan_renderer_amd import capi, feature_buffers, motion_buffers, renderer

f32 = np.float32
U = 2.0 ** -24  # unit roundoff of binary32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cpu_frames(dataset):
    """{extent: dict}: the oracle's visibility and shading data of each frame, its inputs, and the restatement's images for
    every mesh; computed once, left unchanged"""
    out = {}
    for extent in cases.EXTENTS:
        scene = renderer.HostScene()
        try:
            frames.apply_frame(scene, dataset, extent[0], extent[1])
            frame, inputs = frames.oracle_frame(scene)
            out[extent] = dict(inputs=inputs, data=frames.shading_data(frame), second=frames.second_matrix(scene),
                               meshes={name: cases.expected(scene, inputs["visibility"], name) for name in cases.MESHES})
        finally:
            scene.close()
    return out


def test_restated_position_equals_the_oracle_in_every_bit(cpu_frames):
    """P of the restatement - decode_position(), the pixel ray, the barycentrics of intersect_primitive() and the fma chain
    - against the position of oracle_shading_data(), at every covered pixel of every frame"""
    for extent, frame in cpu_frames.items():
        inputs = frame["inputs"]
        P, Q, covered = motion_buffers.positions(inputs["visibility"], inputs["quantized_positions"], None, inputs["constants"])
        assert covered.any() and np.array_equal(covered, inputs["visibility"] != 0xFFFFFFFF)
        different = (P.view(np.uint32) != frame["data"][..., 0:3].view(np.uint32)).any(axis=-1) & covered
        assert not different.any(), (extent, np.argwhere(different)[:4].tolist())
        assert P[covered].tobytes() == Q[covered].tobytes()


def test_equal_arrays_give_the_feature_buffers_reprojection(cpu_frames):
    for extent, frame in cpu_frames.items():
        inputs = frame["inputs"]
        words = inputs["quantized_positions"]
        want = feature_buffers.expected_images(frame["data"], inputs["visibility"], inputs["material_indices"], inputs["constants"], frame["second"])["reprojection"]
        for previous in (None, words, words.copy()):
            got = motion_buffers.expected_images(inputs["visibility"], words, previous, inputs["constants"], frame["second"])
            assert got["reprojection"].tobytes() == want.tobytes(), extent
        assert frame["meshes"]["still"][0]["reprojection"].tobytes() == want.tobytes()


def test_meshes_meet_their_conditions(cpu_frames):
    results = {(name, extent): frame["meshes"][name][:2] + (frame["inputs"]["visibility"],) for extent, frame in cpu_frames.items() for name in cases.MESHES}
    cases.assert_conditions(results)
    words = cpu_frames[(83, 45)]["inputs"]["quantized_positions"]
    for name in cases.MESHES:
        previous, exact = cases.displaced(words, name)
        assert previous.shape == words.shape and (previous.tobytes() == words.tobytes()) == (name == "still")
        # the ground spans the box: a shift bends some triangles; the rigid one, which lifts the ground, leaves most as they are
        assert exact.all() == (name == "still"), name
        assert name != "rigid" or exact.sum() > 0.9 * len(exact), int(exact.sum())


def test_rigid_translation_moves_every_point_by_it(cpu_frames):
    """The mesh moved by d since the previous frame (the previous codes are the current ones plus RIGID_SHIFT: d = -RIGID_SHIFT
    * factor): Q - P = -d at every pixel whose triangle the clipping left alone.

    The bound, from the operations.  With the float32 barycentrics b_i as they are, P = fma(b0, v0, fma(b1, v1, fl(v2 b2)))
    rounds three times, each time by at most U times the magnitude of a partial sum, which S_P = sum |b_i| |v_i| bounds:
    |P - sum b_i v_i| <= 3 U S_P, likewise Q with the previous vertices w_i.  The decoded vertices are rounded once each
    (fma(code, factor, summand)): w_i - v_i = -d +- U (|v_i| + |w_i|), so sum b_i (w_i - v_i) = -d sum b_i +- U (S_P + S_Q).
    Together |(Q - P) + d| <= 4 U (S_P + S_Q) + |d| |sum b_i - 1|, first order in U; the test allows 1 % more for the rest.
    The left side and the sums are evaluated per pixel in binary64."""
    total, largest = 0, 0.0
    for extent, frame in cpu_frames.items():
        inputs = frame["inputs"]
        words, constants, visibility = inputs["quantized_positions"], inputs["constants"], inputs["visibility"]
        previous, exact = cases.displaced(words, "rigid")
        factor, summand = motion_buffers.dequantization(constants)
        d = -(cases.RIGID_SHIFT.astype(np.float64) * factor.astype(np.float64))
        P, Q, covered = motion_buffers.positions(visibility, words, previous, constants)
        now, before = motion_buffers.decode_positions(words, factor, summand), motion_buffers.decode_positions(previous, factor, summand)
        camera = feature_buffers.camera_position(constants)
        rays = motion_buffers.pixel_ray_directions(constants, extent[0], extent[1])
        for y, x in np.argwhere(covered):
            primitive = visibility[y, x]
            if not exact[primitive]:
                continue
            b = motion_buffers.barycentrics(now[primitive], rays[y, x], camera).astype(np.float64)
            v, w = now[primitive].astype(np.float64), before[primitive].astype(np.float64)
            S = (np.abs(b)[:, None] * (np.abs(v) + np.abs(w))).sum(axis=0)
            bound = 1.01 * (4.0 * U * S + np.abs(d) * abs(b.sum() - 1.0))
            error = np.abs((Q[y, x].astype(np.float64) - P[y, x].astype(np.float64)) + d)
            assert (error <= bound).all(), (extent, x, y, error, bound)
            total, largest = total + 1, max(largest, float((error / bound).max()))
        assert exact[visibility[covered]].mean() > 0.9, extent
    print("%d pixels, largest error over bound %.3f" % (total, largest))
    assert total > 900 and np.abs(d).min() > 1.0e-3


def test_ctypes_mirror():
    header = open(os.path.join(ROOT, "include", "vkr_motion_buffers.h")).read()
    struct = re.search(r"typedef struct motion_buffers_s \{(.*?)\} motion_buffers_t;", header, re.S).group(1)
    members = re.findall(r"^\s*(?:const )?(?:void\*|float) (\w+)", struct, re.M)
    assert members == [name for name, _ in capi.MotionBuffers._fields_] == ["previous_positions", "previous_matrix"] + list(capi.MOTION_IMAGES)
    assert C.sizeof(capi.MotionBuffers) == 8 + 64 + 8 * len(capi.MOTION_IMAGES)
    assert capi.MotionBuffers.previous_matrix.offset == 8 and capi.MotionBuffers.reprojection.offset == 72
    lib = capi.load()
    assert "VKR_API int render_motion_buffers(" in header and hasattr(lib, "render_motion_buffers") and "render_motion_buffers" in capi.SIGNATURES
    history_header = open(os.path.join(ROOT, "include", "vkr_frame_history.h")).read()
    assert "VKR_API int accumulate_moving_frame_history(" in history_header
    assert hasattr(lib, "accumulate_moving_frame_history") and len(capi.SIGNATURES["accumulate_moving_frame_history"][1]) == 5


def test_refusals_that_need_no_device(capfd):
    lib = capi.load()

    def one_line(call, function):
        flush_c_output()
        capfd.readouterr()
        result = call()
        flush_c_output()
        printed = capfd.readouterr().out
        assert result == 1 and printed.count("\n") == 1 and printed.startswith(function + "()"), printed

    app, buffers = capi.Application(), capi.MotionBuffers()
    buffers.reprojection = 4096
    # no application, no request, no pass
    one_line(lambda: lib.render_motion_buffers(None, C.byref(buffers)), "render_motion_buffers")
    one_line(lambda: lib.render_motion_buffers(C.byref(app), None), "render_motion_buffers")
    one_line(lambda: lib.render_motion_buffers(C.byref(app), C.byref(buffers)), "render_motion_buffers")
    # the history: checked before anything is queued
    history, settings = capi.FrameHistory(), capi.FrameHistorySettings(32.0, 0.02, 0.9, 4)
    images = capi.FrameHistoryImages(4096, 8192, 12288, None, None, 16384, None)
    name = "accumulate_moving_frame_history"
    one_line(lambda: lib.accumulate_moving_frame_history(None, C.byref(app), C.byref(settings), C.byref(images), 20480), name)
    one_line(lambda: lib.accumulate_moving_frame_history(C.byref(history), C.byref(app), C.byref(capi.FrameHistorySettings(0.5, 0.02, 0.9, 4)), C.byref(images), 20480), name)
    one_line(lambda: lib.accumulate_moving_frame_history(C.byref(history), C.byref(app), C.byref(settings), C.byref(images), 20480 + 8), name)
    # (a history that was not created)
    one_line(lambda: lib.accumulate_moving_frame_history(C.byref(history), C.byref(app), C.byref(settings), C.byref(images), 20480), name)
    one_line(lambda: lib.accumulate_frame_history(C.byref(history), C.byref(app), C.byref(settings), C.byref(images)), "accumulate_frame_history")
    assert history.frame_count == 0 and history.current == 0
