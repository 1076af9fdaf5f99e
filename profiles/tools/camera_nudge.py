#!/usr/bin/env python3
"""The frame of config 3 with a camera that moves before every frame: set_camera (a nudge along x and a small turn) and
render_shading_pass, 500 frames, three frames in flight, wall clock per frame.  The visibility buffer is rendered once
and stays (a caller that rasterises elsewhere and is a frame late): the camera's bytes alone make every light shaft verdict
of the frame before stale, so every pair is walked in every frame - the case that kept verdicts must not make slower.
Prints one JSON line.
  VKR_SHADING_LIBRARY=... python profiles/tools/camera_nudge.py [frames] [large]"""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from vulkan_renderer_amd import renderer, synthetic  # noqa: E402


def main():
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 500
    large = len(sys.argv) > 2 and sys.argv[2] == "large"
    cam = synthetic.DEFAULT_CAMERA
    with tempfile.TemporaryDirectory() as d:
        if large:
            dataset = synthetic.write_dataset(d, seed=4321, ltc_resolution=64, fresnel_count=51, large={})
        else:
            dataset = synthetic.write_dataset(d, grid=256, box_count=64, seed=1234, ltc_resolution=64, fresnel_count=51)
        r = renderer.Renderer(frames_in_flight=3, timing_stride=1 << 30)
        renderer.setup_config(r, 3, dataset, acceleration_structure="sah_device")
        r.create_targets()
        r.create_pass()
        r.render_visibility()

        def run(count, first):
            for k in range(first, first + count):
                r.set_camera((cam["position"][0] + 1.0e-5 * k, cam["position"][1], cam["position"][2]), cam["rotation_x"], cam["rotation_z"] + 1.0e-6 * k,
                             cam["vertical_fov"], cam["near"], cam["far"])
                r.render()
            r.finish_frames()
            r.sync()
        run(200, 0)  # clocks, allocations
        periods = []
        for repeat in range(3):
            start = time.perf_counter()
            run(frames, 200 + repeat * frames)
            periods.append((time.perf_counter() - start) * 1.0e3 / frames)
        stats = r.light_shaft_statistics()
        rays = r.last_ray_count()
        r.close()
    print(json.dumps({"workload": "config 3, camera nudged before every frame", "scene": "large" if large else "bench", "frames": frames, "library": os.environ.get("VKR_SHADING_LIBRARY", "default"),
                      "shaft_rest": os.environ.get("VKR_SHAFT_REST", "default"), "ms_per_frame": [round(p, 4) for p in periods], "rays_last_frame": rays, "resting_pairs_last_frame": stats["not_clear"]["other"]}))


if __name__ == "__main__":
    main()
