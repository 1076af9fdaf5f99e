#!/usr/bin/env python3
"""The shading kernel of config 3 (or the target shape) in its three instantiations, in turn, in one process: HIP events
around the kernel (get_shading_kernel_milliseconds), one frame in flight, animated noise.  A round nudges the camera (the
visibility buffer stays), which makes the next launch plain and the one after it storing; the launches after that load.
Every frame is waited for, so the modes are plain, storing, loading x n per round.  Prints one JSON line (the last line of
its output: the library prints the scene's triangle count before it).
  python profiles/tools/prepared_polygons.py [config] [rounds] [loading frames per round]"""
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from vulkan_renderer_amd import renderer, synthetic  # noqa: E402


def main():
    config = sys.argv[1] if len(sys.argv) > 1 else "3"
    config = int(config) if config.isdigit() else config
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    loading = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    cam = synthetic.DEFAULT_CAMERA
    with tempfile.TemporaryDirectory() as d:
        dataset = synthetic.write_dataset(d, grid=256, box_count=64, seed=1234, ltc_resolution=64, fresnel_count=51)
        r = renderer.Renderer(frames_in_flight=1, timing_stride=1)
        renderer.setup_config(r, config, dataset, acceleration_structure="sah_device", animate_noise=True)
        r.create_targets()
        r.create_pass()
        r.render_visibility()
        times = {"plain": [], "storing": [], "loading": []}
        for k in range(rounds + 2):
            r.set_camera((cam["position"][0] + 1.0e-5 * k, cam["position"][1], cam["position"][2]), cam["rotation_x"], cam["rotation_z"], cam["vertical_fov"], cam["near"], cam["far"])
            for frame in range(2 + loading):
                r.render()
                r.sync()
                mode = r.prepared_polygon_statistics()["mode"]
                # (the first two rounds: clocks, allocations)
                if k >= 2:
                    times[mode].append(r.shading_kernel_ms(1)[-1])
        stats = r.prepared_polygon_statistics()
        r.close()
    out = {"workload": "config %s, shade_pixels alone (HIP events), one frame in flight" % config, "rounds": rounds, "launches": stats["launches"], "buffer_mib": round(stats["buffer_bytes"] / 1048576.0, 1)}
    for mode, values in times.items():
        if values:
            out[mode] = {"n": len(values), "median_ms": round(statistics.median(values), 4), "min_ms": round(min(values), 4), "max_ms": round(max(values), 4)}
    if times["plain"] and times["loading"]:
        out["loading_over_plain"] = round(statistics.median(times["loading"]) / statistics.median(times["plain"]), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
