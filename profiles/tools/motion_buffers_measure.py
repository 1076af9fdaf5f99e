"""Measures render_motion_buffers() (include/vkr_motion_buffers.h) and accumulate_moving_frame_history()
(include/vkr_frame_history.h) on the benchmark scene under config 3 at 1920x1080: the kernel time of the motion images next to
render_feature_buffers() with position and reprojection, against the byte floor; the time of a history call with and without
previous_position for a camera that stands still and one that turns; and what a history is worth while the mesh wobbles - the
error of one frame, of eight accumulated frames with the camera-only reprojection and with the motion buffers, filtered and
not, against a 1024-frame mean of the last pose, and the share of covered pixels without history per frame.  Writes one JSON
record (profiles/r33/motion_buffers.json is a run of it on an MI355X).

    python profiles/tools/motion_buffers_measure.py OUT.json [--quick]

Kernel times follow profiles/tools/feature_buffers_measure.py (HIP events around `--repeats` calls queued back to back while
frames of the pass keep the stream busy, the median of three rounds), history calls and the quality table
profiles/tools/frame_history_measure.py (50 calls back to back, the median of three rounds; RMSE over R, G, B)."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import tempfile


ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from frame_history_measure import FILTER_SETTINGS, HBM_BYTES_PER_SECOND, SCENE, SETTINGS, TURN_PER_FRAME, Images, hip_runtime, open_renderer, turn  # noqa: E402
from vulkan_renderer_amd import feature_buffers, scene_update  # noqa: E402

FEATURES = ("position", "normal", "diffuse_albedo", "reprojection")
MOTION = ("motion_reprojection", "previous_position", "motion")
ACCUMULATED_FRAMES = 8
AMPLITUDE = 0.05
# of the quality table: scene_update's default, and a fifth of it
QUALITY_AMPLITUDES = (0.05, 0.01)


def events(hip):
    start, end = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(start)) == 0 and hip.hipEventCreate(C.byref(end)) == 0
    return start, end


def elapsed(hip, start, end):
    hip.hipEventSynchronize(end)
    ms = C.c_float()
    hip.hipEventElapsedTime(C.byref(ms), start, end)
    return ms.value


def measure_kernels(r, hip, repeats, blockers):
    """The motion images and the feature images of the renderer's frame, the previous positions a wobbled copy on the device"""
    e = r.app.swapchain.extent
    pixels = e.width * e.height
    images = Images(r, hip, FEATURES + MOTION)
    matrix = feature_buffers.world_to_projection_space(r.constants())
    words = scene_update.Wobble(r, AMPLITUDE).words(0)
    previous = C.c_void_p()
    assert hip.hipMalloc(C.byref(previous), words.nbytes) == 0 and hip.hipMemcpy(previous, words.ctypes.data, words.nbytes, 1) == 0
    start, end = events(hip)
    stream = r.app.device.stream
    motion_pointers = {"reprojection": images["motion_reprojection"], "previous_position": images["previous_position"], "motion": images["motion"]}
    requests = {
        "motion_all_three": (3, lambda: r.render_motion(previous.value, matrix, pointers=motion_pointers)),
        "motion_reprojection_alone": (1, lambda: r.render_motion(previous.value, matrix, ["reprojection"], pointers=motion_pointers)),
        "features_position_and_reprojection": (2, lambda: r.render_features(["position", "reprojection"], matrix, pointers=images.features())),
    }
    out = {"width": e.width, "height": e.height, "covered_share": float((r.read_visibility() != 0xFFFFFFFF).mean()), "requests": {}}
    for request, (count, call) in requests.items():
        for _ in range(3):
            call()
        times = []
        for _ in range(3):
            r.sync()
            for _ in range(blockers):
                r.render()
            hip.hipEventRecord(start, stream)
            for _ in range(repeats):
                call()
            hip.hipEventRecord(end, stream)
            times.append(elapsed(hip, start, end) / repeats)
        # per pixel 4 B of visibility, 48 B of vertices (24 now, 24 before; the feature kernel reads 24 and its normals) and
        # 16 B per image
        floor_bytes = pixels * (4 + 48 + 16 * count)
        floor_ms = floor_bytes / HBM_BYTES_PER_SECOND * 1.0e3
        median = statistics.median(times)
        out["requests"][request] = {"images": count, "milliseconds": median, "fastest_milliseconds": min(times), "floor_bytes": floor_bytes,
                                    "floor_milliseconds": floor_ms, "times_the_floor": median / floor_ms}
    r.sync()
    hip.hipFree(previous)
    images.free()
    return out


def measure_history_calls(r, hip, repeats):
    """accumulate_frame_history() and accumulate_moving_frame_history() on the same frame: a camera that stands still and one
    that turned, with out_variance (spatial length 4) and without"""
    e = r.app.swapchain.extent
    pixels = e.width * e.height
    images = Images(r, hip, ("colour",) + FEATURES + ("previous_position", "out_colour", "out_variance"))
    history = r.create_frame_history()
    start, end = events(hip)
    stream = r.app.device.stream
    out = {"width": e.width, "height": e.height, "calls": []}
    for state in ("still", "turning"):
        matrix = turn(r, TURN_PER_FRAME) if state == "turning" else feature_buffers.world_to_projection_space(r.constants())
        r.render(images["colour"])
        r.render_features(list(FEATURES), matrix, pointers=images.features())
        # (nothing moved: previous_position holds this frame's positions, so both calls decide alike and differ by the load)
        r.render_motion(None, matrix, ["previous_position"], pointers={"previous_position": images["previous_position"]})
        r.sync()
        for with_variance in (True, False):
            for moving in (False, True):
                features = dict(images.features(), previous_position=images["previous_position"]) if moving else images.features()

                def call():
                    history.accumulate(images["colour"], features, SETTINGS, out_colour=images["out_colour"], out_variance=images["out_variance"] if with_variance else None)
                for _ in range(8):
                    call()
                times = []
                for _ in range(3):
                    r.sync()
                    hip.hipEventRecord(start, stream)
                    for _ in range(repeats):
                        call()
                    hip.hipEventRecord(end, stream)
                    times.append(elapsed(hip, start, end) / repeats)
                per_pixel = 16 * ((15 if with_variance else 14) + (1 if moving else 0))
                floor_ms = pixels * per_pixel / HBM_BYTES_PER_SECOND * 1.0e3
                median = statistics.median(times)
                out["calls"].append({"state": state, "variance": with_variance, "moving": moving, "milliseconds": median, "fastest_milliseconds": min(times),
                                     "bytes_per_pixel": per_pixel, "floor_milliseconds": floor_ms, "times_the_floor": median / floor_ms})
    history.close()
    images.free()
    return out


def measure_quality(r, hip, reference_frames, amplitude):
    """Eight frames while the mesh wobbles (scene_update's displacement, a step per frame) under a camera that stands still:
    one history with the camera-only reprojection, one with the motion buffers"""
    e = r.app.swapchain.extent
    pixels = e.width * e.height
    images = Images(r, hip, ("colour",) + FEATURES + MOTION[:2] + ("camera_only", "camera_only_variance", "with_motion", "with_motion_variance", "filtered", "reference"))
    histories = {"camera_only": r.create_frame_history(), "with_motion": r.create_frame_history()}
    out = {"frames": ACCUMULATED_FRAMES, "amplitude": amplitude, "reference_frames": reference_frames, "width": e.width, "height": e.height,
           "no_history_share_of_covered": {"camera_only": [], "with_motion": []}}

    def rmse(name):
        return math.sqrt(float(r.squared_error(images[name], images["reference"], pixels).sum()) / (3 * pixels))
    wobble = scene_update.Wobble(r, amplitude)
    matrix = feature_buffers.world_to_projection_space(r.constants())
    previous_words = None
    for index in range(ACCUMULATED_FRAMES):
        words = wobble.words(index)
        r.update_geometry(words)
        r.render_visibility()
        r.render(images["colour"])
        r.render_features(list(FEATURES), matrix, pointers=images.features())
        r.render_motion(previous_words, matrix, ["reprojection", "previous_position"],
                        pointers={"reprojection": images["motion_reprojection"], "previous_position": images["previous_position"]})
        moving = dict(images.features(), reprojection=images["motion_reprojection"], previous_position=images["previous_position"])
        histories["camera_only"].accumulate(images["colour"], images.features(), SETTINGS, out_colour=images["camera_only"], out_variance=images["camera_only_variance"])
        histories["with_motion"].accumulate(images["colour"], moving, SETTINGS, out_colour=images["with_motion"], out_variance=images["with_motion_variance"])
        for key, history in histories.items():
            lengths = history.read()["colour"][..., 3]
            out["no_history_share_of_covered"][key].append(float((lengths[lengths > 0] == 1).mean()))
        previous_words = words
    features = images.features()
    statistics_ = r.create_statistics()
    for _ in range(reference_frames):
        r.render()
        statistics_.accumulate()
    statistics_.resolve(images["reference"], None)
    r.sync()
    statistics_.close()
    out["rmse_one_frame"] = rmse("colour")
    for key in histories:
        out["rmse_" + key] = rmse(key)
        r.filter_frame(images[key], images[key + "_variance"], features, FILTER_SETTINGS, out_colour=images["filtered"])
        r.sync()
        out["rmse_" + key + "_filtered"] = rmse("filtered")
    for history in histories.values():
        history.close()
    images.free()
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("out")
    parser.add_argument("--quick", action="store_true", help="a small scene and few repeats: checks the script, measures nothing")
    parser.add_argument("--repeats", type=int, default=100)
    parser.add_argument("--reference-frames", type=int, default=1024)
    options = parser.parse_args()
    hip = hip_runtime()
    scene = dict(grid=32, box_count=8, ltc_resolution=16, fresnel_count=8) if options.quick else SCENE
    width, height = (320, 180) if options.quick else (1920, 1080)
    record = {"scene": scene, "settings": SETTINGS, "filter_settings": FILTER_SETTINGS}
    with tempfile.TemporaryDirectory() as directory:
        dataset = __import__("vulkan_renderer_amd.synthetic", fromlist=["synthetic"]).write_dataset(os.path.join(directory, "plain"), seed=1234, **scene)
        measures = [("kernels", lambda r: measure_kernels(r, hip, 3 if options.quick else options.repeats, 4 if options.quick else 40)),
                    ("history_calls", lambda r: measure_history_calls(r, hip, 3 if options.quick else options.repeats // 2))]
        measures += [("quality_%g" % amplitude, lambda r, amplitude=amplitude: measure_quality(r, hip, 16 if options.quick else options.reference_frames, amplitude))
                     for amplitude in QUALITY_AMPLITUDES]
        for key, measure in measures:
            r = open_renderer(dataset, width, height, frames_in_flight=3 if key.startswith("quality") else 1)
            if key == "kernels":
                # (as profiles/tools/feature_buffers_measure.py has it: with animated noise every call uploads new constants)
                r.app.render_settings.animate_noise = 0
            try:
                record[key] = measure(r)
            finally:
                r.close()
            print(key, json.dumps(record[key]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(options.out)), exist_ok=True)
    with open(options.out, "w") as file:
        json.dump(record, file, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
