#!/usr/bin/env python3
"""The shading kernel of config 3 (or the target shape) in its four instantiations, in turn, in one process: HIP events
around the kernel (get_shading_kernel_milliseconds), one frame in flight, animated noise.  A round nudges the camera (the
visibility buffer stays), which makes the next launch plain and the one after it storing; the launches after that load.
Every frame is waited for, so the modes are plain, storing, loading x n per round.  The rounds come in blocks that take
turns: one block with the sector terms (the storing step then includes the kernel that fills them, and the launches load
with terms), one without (VKR_SECTOR_TERMS=0, read when the pass is created).  Prints one JSON line (the last line of its
output: the library prints the scene's triangle count before it).
  python profiles/tools/prepared_polygons.py [config] [rounds per block] [loading frames per round] [blocks per kind]
(defaults 5, 8, 3: 15 rounds per kind - the tool of r18 ran 20 rounds of the one kind there was)"""
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from vulkan_renderer_amd import renderer, synthetic  # noqa: E402


def summary(values):
    return {"n": len(values), "median_ms": round(statistics.median(values), 4), "min_ms": round(min(values), 4), "max_ms": round(max(values), 4)}


def main():
    config = sys.argv[1] if len(sys.argv) > 1 else "3"
    config = int(config) if config.isdigit() else config
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    loading = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    blocks = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    cam = synthetic.DEFAULT_CAMERA
    times = {"plain": [], "storing": [], "storing_and_terms": [], "loading": [], "loading_with_terms": []}
    nudge = 0
    terms_mib = 0.0
    launches = {"plain": 0, "storing": 0, "loading": 0}
    loaded = {"loaded_with_terms": 0, "loaded_without_terms": 0}
    with tempfile.TemporaryDirectory() as d:
        dataset = synthetic.write_dataset(d, grid=256, box_count=64, seed=1234, ltc_resolution=64, fresnel_count=51)
        r = renderer.Renderer(frames_in_flight=1, timing_stride=1)
        renderer.setup_config(r, config, dataset, acceleration_structure="sah_device", animate_noise=True)
        r.create_targets()
        for block in range(2 * blocks):
            terms = block % 2 == 0
            os.environ["VKR_SECTOR_TERMS"] = "1" if terms else "0"
            r.sync()
            r.create_pass()
            r.render_visibility()
            for k in range(rounds + 2):
                nudge += 1
                r.set_camera((cam["position"][0] + 1.0e-5 * nudge, cam["position"][1], cam["position"][2]), cam["rotation_x"], cam["rotation_z"], cam["vertical_fov"], cam["near"], cam["far"])
                for frame in range(2 + loading):
                    before = r.sector_terms_statistics()
                    r.render()
                    r.sync()
                    mode = r.prepared_polygon_statistics()["mode"]
                    after = r.sector_terms_statistics()
                    if mode == "loading" and after["loaded_with_terms"] != before["loaded_with_terms"]:
                        mode = "loading_with_terms"
                    elif mode == "storing" and after["buffer_bytes"] != 0:
                        mode = "storing_and_terms"
                    # (the first two rounds of a block: clocks, allocations)
                    if k >= 2:
                        times[mode].append(r.shading_kernel_ms(1)[-1])
            stats, terms_stats = r.prepared_polygon_statistics(), r.sector_terms_statistics()
            # (a pass counts its own launches: summed over the blocks)
            for mode in launches:
                launches[mode] += stats["launches"][mode]
            for kind in loaded:
                loaded[kind] += terms_stats[kind]
            if terms:
                terms_mib = round(terms_stats["buffer_bytes"] / 1048576.0, 1)
        r.close()
    out = {"workload": "config %s, shade_pixels alone (HIP events), one frame in flight" % config, "rounds": rounds * blocks, "launches": dict(launches, **loaded), "buffer_mib": round(stats["buffer_bytes"] / 1048576.0, 1),
           "terms_mib": terms_mib}
    for mode, values in times.items():
        if values:
            out[mode] = summary(values)
    if times["plain"] and times["loading"]:
        out["loading_over_plain"] = round(statistics.median(times["loading"]) / statistics.median(times["plain"]), 4)
    if times["loading_with_terms"] and times["loading"]:
        out["with_terms_over_loading"] = round(statistics.median(times["loading_with_terms"]) / statistics.median(times["loading"]), 4)
    if times["storing_and_terms"] and times["storing"]:
        out["terms_kernel_ms"] = round(statistics.median(times["storing_and_terms"]) - statistics.median(times["storing"]), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
