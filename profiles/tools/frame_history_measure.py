"""Measures accumulate_frame_history() (include/vkr_frame_history.h) on frames of the benchmark scene under config 3: the time
of a call against its byte floor with and without out_variance in three states (a camera that stands still, one that turns,
the first frame after a reset), the frame period of config 3 with three frames in flight with and without a call per frame,
the error of one frame and of eight accumulated frames, filtered and not, against a 1024-frame mean for a still camera and
after a turn, and the share of pixels without history per frame of the turn.  Writes one JSON record
(profiles/r31/frame_history.json is a run of it on an MI355X).

    python profiles/tools/frame_history_measure.py OUT.json [--quick]

Call times are HIP events around `--repeats` calls queued back to back on the device's stream, divided by their number, the
median of three such rounds."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from vulkan_renderer_amd import feature_buffers, frame_filter, frame_history, renderer, synthetic  # noqa: E402

HBM_BYTES_PER_SECOND = 6.3e12  # what a float4 copy reaches on an MI355X
# the compulsory bytes: colour, position, normal, reprojection and modulation in, four history images read once and four
# written, out_colour and, with it, out_variance
BYTES_PER_PIXEL = {True: 15 * 16, False: 14 * 16}
# the first frame of a history reads none
BYTES_PER_PIXEL_WITHOUT_HISTORY = {True: 11 * 16, False: 10 * 16}
SETTINGS = dict(frame_history.DEFAULT_SETTINGS)
FILTER_SETTINGS = dict(frame_filter.DEFAULT_SETTINGS, variance_scale=1.0)
EXTENTS = [(1920, 1080), (3840, 2160)]
SCENE = dict(grid=256, box_count=64, ltc_resolution=64, fresnel_count=51)
FEATURES = ("position", "normal", "diffuse_albedo", "reprojection")
TURN_PER_FRAME = math.radians(0.5)
ACCUMULATED_FRAMES = 8


def hip_runtime():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    return hip


def open_renderer(dataset, width, height, frames_in_flight=1):
    r = renderer.Renderer(frames_in_flight=frames_in_flight, timing_stride=1 << 30)
    renderer.setup_config(r, 3, dataset, width, height, sample_count=1, acceleration_structure=True)
    r.app.render_settings.animate_noise = 1
    r.create_targets()
    r.create_pass()
    r.render_visibility()
    return r


class Images:
    """Device images of the renderer's extent by name"""

    def __init__(self, r, hip, names):
        e = r.app.swapchain.extent
        self.hip, self.shape, self.nbytes, self.pointers = hip, (e.height, e.width, 4), e.width * e.height * 16, {}
        for name in names:
            self.pointers[name] = C.c_void_p()
            assert hip.hipMalloc(C.byref(self.pointers[name]), self.nbytes) == 0

    def __getitem__(self, name):
        return self.pointers[name].value

    def features(self):
        return {name: self[name] for name in FEATURES}

    def free(self):
        for pointer in self.pointers.values():
            self.hip.hipFree(pointer)


def turn(r, angle):
    """-> the matrix of the camera as it was; the camera turned about the vertical axis, the visibility of the new view"""
    matrix = feature_buffers.world_to_projection_space(r.constants())
    r.app.scene_specification.camera.rotation_z += angle
    r.render_visibility()
    return matrix


def render_frame(r, images, previous_matrix=None):
    """A frame into images["colour"] and its features, the reprojection under previous_matrix (None: the frame's own)"""
    r.render(images["colour"])
    r.render_features(list(FEATURES), previous_matrix, pointers=images.features())


def measure_calls(r, hip, repeats):
    e = r.app.swapchain.extent
    pixels = e.width * e.height
    images = Images(r, hip, ("colour",) + FEATURES + ("out_colour", "out_variance"))
    history = r.create_frame_history()
    start, end = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(start)) == 0 and hip.hipEventCreate(C.byref(end)) == 0
    stream = r.app.device.stream
    out = {"width": e.width, "height": e.height, "calls": []}

    def timed(call):
        for _ in range(8):
            call()
        times = []
        for _ in range(3):
            r.sync()
            hip.hipEventRecord(start, stream)
            for _ in range(repeats):
                call()
            hip.hipEventRecord(end, stream)
            hip.hipEventSynchronize(end)
            ms = C.c_float()
            hip.hipEventElapsedTime(C.byref(ms), start, end)
            times.append(ms.value / repeats)
        return times
    for state in ("still", "turning", "reset"):
        if state == "turning":
            render_frame(r, images, turn(r, TURN_PER_FRAME))
        else:
            render_frame(r, images)
        r.sync()
        for with_variance in (True, False):
            for spatial_length in ((SETTINGS["spatial_length"], 0) if with_variance else (SETTINGS["spatial_length"],)):
                settings = dict(SETTINGS, spatial_length=spatial_length)

                def call():
                    if state == "reset":
                        history.reset()
                    history.accumulate(images["colour"], images.features(), settings, out_colour=images["out_colour"],
                                       out_variance=images["out_variance"] if with_variance else None)
                times = timed(call)
                lengths = history.read()["colour"][..., 3]
                covered = lengths > 0
                per_pixel = (BYTES_PER_PIXEL_WITHOUT_HISTORY if state == "reset" else BYTES_PER_PIXEL)[with_variance]
                floor_ms = pixels * per_pixel / HBM_BYTES_PER_SECOND * 1.0e3
                median = statistics.median(times)
                out["calls"].append({"state": state, "variance": with_variance, "spatial_length": spatial_length, "milliseconds": median,
                                     "fastest_milliseconds": min(times), "bytes_per_pixel": per_pixel, "floor_milliseconds": floor_ms,
                                     "times_the_floor": median / floor_ms, "covered_share": float(covered.mean()),
                                     "short_history_share_of_covered": float((lengths[covered] < SETTINGS["spatial_length"]).mean())})
    history.close()
    images.free()
    return out


def measure_frame_period(r, hip, frames, rounds):
    """config 3, three frames in flight: wall clock per frame of `frames` frames, with and without a call on the radiance
    target behind every frame (a camera that stands still), alternating"""
    images = Images(r, hip, ("colour",) + FEATURES + ("out_colour", "out_variance"))
    render_frame(r, images)
    features = images.features()

    def period(with_history):
        r.finish_frames()
        r.sync()
        began = time.perf_counter()
        for _ in range(frames):
            r.render()
            if with_history:
                r.accumulate_history(r.app.render_targets.radiance, features, SETTINGS, out_colour=images["out_colour"], out_variance=images["out_variance"])
        r.finish_frames()
        r.sync()
        return (time.perf_counter() - began) * 1.0e3 / frames
    period(False), period(True)
    without, with_ = [], []
    for _ in range(rounds):
        without.append(period(False))
        with_.append(period(True))
    images.free()
    return {"frames_per_round": frames, "rounds": rounds, "without_milliseconds": without, "with_milliseconds": with_,
            "median_without": statistics.median(without), "median_with": statistics.median(with_)}


def measure_quality(r, hip, reference_frames, turning):
    """RMSE over R, G, B against the mean of `reference_frames` frames of the last camera: the last frame alone, that frame
    filtered (no variance image), ACCUMULATED_FRAMES frames accumulated, and those filtered with the history's variance"""
    e = r.app.swapchain.extent
    pixels = e.width * e.height
    images = Images(r, hip, ("colour",) + FEATURES + ("accumulated", "variance", "filtered", "reference"))
    history = r.create_frame_history()
    out = {"turning": turning, "degrees_per_frame": math.degrees(TURN_PER_FRAME) if turning else 0.0, "frames": ACCUMULATED_FRAMES,
           "reference_frames": reference_frames, "width": e.width, "height": e.height, "no_history_share_of_covered": []}

    def rmse(name):
        return math.sqrt(float(r.squared_error(images[name], images["reference"], pixels).sum()) / (3 * pixels))
    previous = None
    for index in range(ACCUMULATED_FRAMES):
        if index and turning:
            previous = turn(r, TURN_PER_FRAME)
        render_frame(r, images, previous)
        history.accumulate(images["colour"], images.features(), SETTINGS, out_colour=images["accumulated"], out_variance=images["variance"])
        lengths = history.read()["colour"][..., 3]
        out["no_history_share_of_covered"].append(float((lengths[lengths > 0] == 1).mean()))
    features = images.features()
    r.filter_frame(images["colour"], None, features, FILTER_SETTINGS, out_colour=images["filtered"])
    r.sync()
    statistics_ = r.create_statistics()
    for _ in range(reference_frames):
        r.render()
        statistics_.accumulate()
    statistics_.resolve(images["reference"], None)
    r.sync()
    statistics_.close()
    out["rmse_one_frame"], out["rmse_one_frame_filtered"], out["rmse_accumulated"] = rmse("colour"), rmse("filtered"), rmse("accumulated")
    r.filter_frame(images["accumulated"], images["variance"], features, FILTER_SETTINGS, out_colour=images["filtered"])
    r.sync()
    out["rmse_accumulated_filtered"] = rmse("filtered")
    history.close()
    images.free()
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("out")
    parser.add_argument("--quick", action="store_true", help="a small scene and few repeats: checks the script, measures nothing")
    parser.add_argument("--repeats", type=int, default=50)
    parser.add_argument("--reference-frames", type=int, default=1024)
    options = parser.parse_args()
    hip = hip_runtime()
    scene = dict(grid=32, box_count=8, ltc_resolution=16, fresnel_count=8) if options.quick else SCENE
    extents = [(320, 180)] if options.quick else EXTENTS
    with tempfile.TemporaryDirectory() as directory:
        dataset = synthetic.write_dataset(os.path.join(directory, "plain"), seed=1234, **scene)
        record = {"scene": scene, "settings": SETTINGS, "filter_settings": FILTER_SETTINGS, "frames": [], "quality": []}
        for width, height in extents:
            r = open_renderer(dataset, width, height)
            try:
                record["frames"].append(measure_calls(r, hip, 3 if options.quick else options.repeats))
            finally:
                r.close()
            print(width, height, json.dumps(record["frames"][-1]["calls"]), flush=True)
        r = open_renderer(dataset, extents[0][0], extents[0][1], frames_in_flight=3)
        try:
            record["frame_period"] = measure_frame_period(r, hip, 20 if options.quick else 300, 2 if options.quick else 5)
        finally:
            r.close()
        print("frame period", json.dumps(record["frame_period"]), flush=True)
        for turning in (False, True):
            r = open_renderer(dataset, extents[0][0], extents[0][1], frames_in_flight=3)
            try:
                record["quality"].append(measure_quality(r, hip, 16 if options.quick else options.reference_frames, turning))
            finally:
                r.close()
            print("quality", json.dumps(record["quality"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(options.out)), exist_ok=True)
    with open(options.out, "w") as file:
        json.dump(record, file, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
