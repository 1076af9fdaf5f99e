"""Measures render_feature_buffers() (include/vkr_feature_buffers.h) on the benchmark scene: the kernel time of three
requests against their byte floors, against what a caller had to do before (pixel_rays() + trace_closest_hits() + a
read-back), the same on a textured scene, and the frame period of config 3 with three frames in flight with and without a
feature call per frame.  Writes one JSON record (profiles/r29/feature_buffers.json is a run of it on an MI355X).

    python profiles/tools/feature_buffers_measure.py OUT.json [--quick]

Kernel times are HIP events around `--repeats` calls queued back to back on the device's stream while earlier frames keep
it busy, divided by their number, the median of three such rounds; a run under `rocprofv3 --kernel-trace --stats` shows the
same kernels by name (k_feature_buffers<false / true>)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from vulkan_renderer_amd import capi, renderer, synthetic  # noqa: E402

HBM_BYTES_PER_SECOND = 6.3e12  # what a float4 copy reaches on an MI355X (79 % of the 8 TB/s of the specification)
REQUESTS = {"denoiser_set": ("position", "normal", "diffuse_albedo"), "all_seven": capi.PIXEL_FEATURES, "identity_alone": ("identity",)}


def hip_runtime():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    return hip


def measure_requests(r, hip, repeats, blockers):
    """-> {request: milliseconds, floors, ...} for the renderer's current frame"""
    e = r.app.swapchain.extent
    pixels = e.width * e.height
    visibility = r.read_visibility()
    covered = visibility != 0xFFFFFFFF
    distinct = len(np.unique(visibility[covered]))
    buffers = {}
    for name in capi.PIXEL_FEATURES:
        buffers[name] = C.c_void_p()
        assert hip.hipMalloc(C.byref(buffers[name]), pixels * 16) == 0
    start, end = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(start)) == 0 and hip.hipEventCreate(C.byref(end)) == 0
    stream = r.app.device.stream
    out = {"width": e.width, "height": e.height, "covered_share": float(covered.mean()), "distinct_primitives": distinct, "requests": {}}
    for request, names in REQUESTS.items():
        pointers = {name: buffers[name].value for name in names}
        for _ in range(3):
            r.render_features(names, pointers=pointers)
        times = []
        for _ in range(3):
            r.sync()
            # frames of the pass keep the stream busy while the host queues the calls: the events then see the kernels back
            # to back and nothing of the host
            for _ in range(blockers):
                r.render()
            hip.hipEventRecord(start, stream)
            for _ in range(repeats):
                r.render_features(names, pointers=pointers)
            hip.hipEventRecord(end, stream)
            hip.hipEventSynchronize(end)
            ms = C.c_float()
            hip.hipEventElapsedTime(C.byref(ms), start, end)
            times.append(ms.value / repeats)
        # per pixel 16 B per image and 4 B of visibility; per distinct primitive its three vertices (2 x 8 B each) and its
        # material index, once
        floor_bytes = pixels * (16 * len(names) + 4) + distinct * (3 * 16 + 1)
        floor_ms = floor_bytes / HBM_BYTES_PER_SECOND * 1.0e3
        median = statistics.median(times)
        out["requests"][request] = {"images": len(names), "milliseconds": median, "fastest_milliseconds": min(times), "floor_bytes": floor_bytes,
                                    "floor_milliseconds": floor_ms, "share_of_floor": floor_ms / median,
                                    "bound_by": "memory (within 2x of the byte floor)" if median < 2.0 * floor_ms else "latency and arithmetic (more than 2x the byte floor)"}
    # what a caller did before: the pixel rays, closest hits with (primitive, t, u, v), and the answers read back
    times = []
    for _ in range(3):
        began = time.perf_counter()
        rays = r.pixel_rays()
        hits = r.trace_closest_hits(rays["origin"], rays["direction"], rays["t_min"], rays["t_max"], cull_back_faces=True)
        times.append((time.perf_counter() - began) * 1.0e3)
    out["pixel_rays_and_closest_hits_milliseconds"] = min(times)
    out["closest_hit_bytes_read_back"] = int(hits.nbytes)
    for pointer in buffers.values():
        hip.hipFree(pointer)
    return out


def measure_frame_period(r, hip, frames, rounds):
    """config 3, three frames in flight: wall clock per frame of `frames` frames, with and without a feature call (the
    denoiser set, to device memory) behind every frame, alternating"""
    e = r.app.swapchain.extent
    names = REQUESTS["denoiser_set"]
    buffers = {name: C.c_void_p() for name in names}
    for pointer in buffers.values():
        assert hip.hipMalloc(C.byref(pointer), e.width * e.height * 16) == 0
    pointers = {name: pointer.value for name, pointer in buffers.items()}

    def period(with_features):
        r.finish_frames()
        r.sync()
        began = time.perf_counter()
        for _ in range(frames):
            r.render()
            if with_features:
                r.render_features(names, pointers=pointers)
        r.finish_frames()
        r.sync()
        return (time.perf_counter() - began) * 1.0e3 / frames
    period(False), period(True)
    without, with_ = [], []
    for _ in range(rounds):
        without.append(period(False))
        with_.append(period(True))
    for pointer in buffers.values():
        hip.hipFree(pointer)
    return {"frames_per_round": frames, "rounds": rounds, "without_milliseconds": without, "with_milliseconds": with_,
            "median_without": statistics.median(without), "median_with": statistics.median(with_)}


def open_renderer(dataset, width, height, frames_in_flight=1):
    r = renderer.Renderer(frames_in_flight=frames_in_flight, timing_stride=1 << 30)
    renderer.setup_config(r, 3, dataset, width, height, acceleration_structure=True)
    r.create_targets()
    r.create_pass()
    r.render_visibility()
    return r


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("out")
    parser.add_argument("--quick", action="store_true", help="a small scene and few repeats: checks the script, measures nothing")
    parser.add_argument("--repeats", type=int, default=100)
    options = parser.parse_args()
    hip = hip_runtime()
    scene = dict(grid=32, box_count=8, ltc_resolution=16, fresnel_count=8) if options.quick else dict(grid=256, box_count=64, ltc_resolution=64, fresnel_count=51)
    extents = [(320, 180)] if options.quick else [(1920, 1080), (3840, 2160)]
    repeats = 3 if options.quick else options.repeats
    record = {"scene": scene, "frames": [], "textured_frames": []}
    with tempfile.TemporaryDirectory() as directory:
        dataset = synthetic.write_dataset(os.path.join(directory, "plain"), seed=1234, **scene)
        textured = synthetic.write_dataset(os.path.join(directory, "textured"), seed=1234, textured=True, texture_size=64 if options.quick else 256, **scene)
        for width, height in extents:
            for source, key in ((dataset, "frames"), (textured, "textured_frames")):
                r = open_renderer(source, width, height)
                try:
                    record[key].append(measure_requests(r, hip, repeats, 4 if options.quick else (40 if width <= 1920 else 15)))
                finally:
                    r.close()
                print(key, width, height, json.dumps(record[key][-1]["requests"]), flush=True)
        r = open_renderer(dataset, extents[0][0], extents[0][1], frames_in_flight=3)
        try:
            record["frame_period"] = measure_frame_period(r, hip, 20 if options.quick else 300, 2 if options.quick else 5)
        finally:
            r.close()
        print("frame period", json.dumps(record["frame_period"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(options.out)), exist_ok=True)
    with open(options.out, "w") as file:
        json.dump(record, file, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
