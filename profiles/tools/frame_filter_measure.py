"""Measures filter_frame() (include/vkr_frame_filter.h) on frames of the benchmark scene under config 3: the time of a call
of one to five iterations against the byte floor, each launch's own time from a kernel trace, the frame period of config 3
with three frames in flight with and without a five-iteration call per frame, and what the filter does to the error of a
one-frame image.  Writes one JSON record (profiles/r30/frame_filter.json is a run of it on an MI355X).

    python profiles/tools/frame_filter_measure.py OUT.json [--quick]
    rocprofv3 --kernel-trace --output-format csv -d TRACE_DIR -- python profiles/tools/frame_filter_measure.py --trace-run
    python profiles/tools/frame_filter_measure.py OUT.json --merge-trace TRACE_DIR

Call times are HIP events around `--repeats` calls queued back to back on the device's stream, divided by their number, the
median of three such rounds.  The trace run queues ten five-iteration calls per extent, with and without a variance image;
--merge-trace takes the median duration of each launch (the n-th k_filter_* kernel of every call) into OUT.json."""
import argparse
import csv
import ctypes as C
import glob
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
from vulkan_renderer_amd import frame_filter, renderer, synthetic  # noqa: E402

HBM_BYTES_PER_SECOND = 6.3e12  # what a float4 copy reaches on an MI355X
# colour, variance, position and normal in, colour and variance out; without a variance image 64
BYTES_PER_PIXEL = {True: 96, False: 64}
SETTINGS = dict(frame_filter.DEFAULT_SETTINGS)
EXTENTS = [(1920, 1080), (3840, 2160)]
SCENE = dict(grid=256, box_count=64, ltc_resolution=64, fresnel_count=51)
TRACE_CALLS = 10


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

    def download(self, name):
        out = np.zeros(self.shape, np.float32)
        assert self.hip.hipMemcpy(out.ctypes.data, self.pointers[name], self.nbytes, 2) == 0
        return out

    def free(self):
        for pointer in self.pointers.values():
            self.hip.hipFree(pointer)


def prepare_inputs(r, images, frame_count):
    """mean and variance of `frame_count` frames, position, normal and albedo of the frame"""
    statistics_ = r.create_statistics()
    for _ in range(frame_count):
        r.render()
        statistics_.accumulate()
    statistics_.resolve(images["mean"], images["variance"] if frame_count >= 2 else None)
    features = {name: images[name] for name in ("position", "normal", "diffuse_albedo")}
    r.render_features(list(features), pointers=features)
    r.sync()
    statistics_.close()
    return features


def measure_calls(r, hip, repeats):
    """-> the time of filter_frame() for 1 ... 5 iterations, with and without a variance image, on a four-frame mean"""
    e = r.app.swapchain.extent
    pixels = e.width * e.height
    images = Images(r, hip, ("mean", "variance", "position", "normal", "diffuse_albedo", "out_colour", "out_variance"))
    features = prepare_inputs(r, images, 4)
    covered = float((images.download("position")[..., 3] > 0).mean())
    start, end = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(start)) == 0 and hip.hipEventCreate(C.byref(end)) == 0
    stream = r.app.device.stream
    out = {"width": e.width, "height": e.height, "covered_share": covered, "calls": []}
    for with_variance in (True, False):
        for n in range(1, 6):
            settings = dict(SETTINGS, iteration_count=n, variance_scale=0.25)

            def call():
                r.filter_frame(images["mean"], images["variance"] if with_variance else None, features, settings, out_colour=images["out_colour"],
                               out_variance=images["out_variance"] if with_variance else None)
            for _ in range(3):
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
            floor_ms = n * pixels * BYTES_PER_PIXEL[with_variance] / HBM_BYTES_PER_SECOND * 1.0e3
            median = statistics.median(times)
            out["calls"].append({"variance": with_variance, "iterations": n, "milliseconds": median, "fastest_milliseconds": min(times),
                                 "floor_milliseconds": floor_ms, "times_the_floor": median / floor_ms})
    images.free()
    return out


def measure_frame_period(r, hip, frames, rounds):
    """config 3, three frames in flight: wall clock per frame of `frames` frames, with and without a five-iteration
    filter_frame() of the radiance target behind every frame, alternating"""
    images = Images(r, hip, ("mean", "variance", "position", "normal", "diffuse_albedo", "out_colour"))
    features = prepare_inputs(r, images, 2)
    settings = dict(SETTINGS, variance_scale=1.0)

    def period(with_filter):
        r.finish_frames()
        r.sync()
        began = time.perf_counter()
        for _ in range(frames):
            r.render()
            if with_filter:
                r.filter_frame(r.app.render_targets.radiance, images["variance"], features, settings, out_colour=images["out_colour"])
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


def measure_quality(r, hip, reference_frames):
    """RMSE over R, G, B of a one-frame image (no variance: no luminance weight) and of a four-frame mean with its variance,
    unfiltered and filtered, against the mean of `reference_frames` frames"""
    e = r.app.swapchain.extent
    pixels = e.width * e.height
    images = Images(r, hip, ("mean", "variance", "position", "normal", "diffuse_albedo", "out_colour", "reference"))
    statistics_ = r.create_statistics()
    for _ in range(reference_frames):
        r.render()
        statistics_.accumulate()
    statistics_.resolve(images["reference"], None)
    r.sync()
    statistics_.close()
    out = {"reference_frames": reference_frames, "width": e.width, "height": e.height, "settings": SETTINGS, "images": []}

    def rmse(name):
        return math.sqrt(float(r.squared_error(images[name], images["reference"], pixels).sum()) / (3 * pixels))
    for frame_count in (1, 4):
        features = prepare_inputs(r, images, frame_count)
        settings = dict(SETTINGS, variance_scale=1.0 / frame_count)
        r.filter_frame(images["mean"], images["variance"] if frame_count >= 2 else None, features, settings, out_colour=images["out_colour"])
        out["images"].append({"frames": frame_count, "variance_image": frame_count >= 2, "rmse_unfiltered": rmse("mean"), "rmse_filtered": rmse("out_colour")})
    images.free()
    return out


def trace_run(dataset, hip):
    """What the kernel trace is taken of: per extent TRACE_CALLS five-iteration calls with a variance image, then as many
    without, after three of each that warm up (dropped by --merge-trace)"""
    for width, height in EXTENTS:
        r = open_renderer(dataset, width, height)
        images = Images(r, hip, ("mean", "variance", "position", "normal", "diffuse_albedo", "out_colour", "out_variance"))
        try:
            features = prepare_inputs(r, images, 4)
            for with_variance in (True, False):
                for _ in range(3 + TRACE_CALLS):
                    r.filter_frame(images["mean"], images["variance"] if with_variance else None, features, dict(SETTINGS, variance_scale=0.25),
                                   out_colour=images["out_colour"], out_variance=images["out_variance"] if with_variance else None)
                r.sync()
        finally:
            images.free()
            r.close()


def merge_trace(record, directory):
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as file:
            rows += [row for row in csv.DictReader(file) if "k_filter_" in row["Kernel_Name"]]
    rows.sort(key=lambda row: int(row["Start_Timestamp"]))
    per_group = 5 * (3 + TRACE_CALLS)
    assert len(rows) == per_group * 2 * len(EXTENTS), len(rows)
    record["launches"] = []
    for index, (width, height) in enumerate(EXTENTS):
        for v, with_variance in enumerate((True, False)):
            group = rows[(2 * index + v) * per_group:][:per_group][5 * 3:]
            floor_us = width * height * BYTES_PER_PIXEL[with_variance] / HBM_BYTES_PER_SECOND * 1.0e6
            for i in range(5):
                launches = group[i::5]
                microseconds = statistics.median((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1.0e3 for row in launches)
                first = launches[0]
                record["launches"].append({"width": width, "height": height, "variance": with_variance, "iteration": i, "step": 1 << i,
                                           "kernel": first["Kernel_Name"], "microseconds": microseconds, "floor_microseconds": floor_us,
                                           "times_the_floor": microseconds / floor_us,
                                           "lds_bytes": first.get("LDS_Block_Size"), "scratch_bytes": first.get("Scratch_Size")})


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("out", nargs="?")
    parser.add_argument("--quick", action="store_true", help="a small scene and few repeats: checks the script, measures nothing")
    parser.add_argument("--repeats", type=int, default=50)
    parser.add_argument("--reference-frames", type=int, default=1024)
    parser.add_argument("--trace-run", action="store_true")
    parser.add_argument("--merge-trace", metavar="DIR")
    options = parser.parse_args()
    if options.merge_trace:
        with open(options.out) as file:
            record = json.load(file)
        merge_trace(record, options.merge_trace)
        with open(options.out, "w") as file:
            json.dump(record, file, indent=1)
        return 0
    hip = hip_runtime()
    scene = dict(grid=32, box_count=8, ltc_resolution=16, fresnel_count=8) if options.quick else SCENE
    extents = [(320, 180)] if options.quick else EXTENTS
    with tempfile.TemporaryDirectory() as directory:
        dataset = synthetic.write_dataset(os.path.join(directory, "plain"), seed=1234, **scene)
        if options.trace_run:
            trace_run(dataset, hip)
            return 0
        record = {"scene": scene, "settings": SETTINGS, "frames": []}
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
        r = open_renderer(dataset, extents[0][0], extents[0][1], frames_in_flight=3)
        try:
            record["quality"] = measure_quality(r, hip, 16 if options.quick else options.reference_frames)
        finally:
            r.close()
        print("quality", json.dumps(record["quality"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(options.out)), exist_ok=True)
    with open(options.out, "w") as file:
        json.dump(record, file, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
