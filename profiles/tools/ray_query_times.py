#!/usr/bin/env python3
"""Times of the ray queries (include/vkr_ray_queries.h) on the 1920x1080 benchmark view of the benchmark scene and of the
large scene: closest hit (two-sided, culled) and any hit, with the binary walk, the wide walk and `auto`, on three ray
sets -

  raster    the pixel-centre rays of the camera in raster order (2.07 M)
  shuffled  the same rays in random order
  cosine    one cosine-distributed ray from every visible point, t in [1e-3, 2]

- next to render_visibility_pass() on the same view, which is the closest-hit code that existed before (it generates its
rays and writes 4 bytes per pixel; a closest-hit query reads 32 and writes 16 bytes per ray).

One process; HIP events around the enqueued call on the device's stream; WARMUP untimed rounds, then REPEATS rounds in
which every variant of a group runs once, one after the other, so that what is compared is measured alternately; the
median per variant, with the smallest and the largest time.  `auto` runs the same kernel as one of the forced walks: the
difference between these two is the spread of identical runs.

    python profiles/tools/ray_query_times.py --out DIR [--scenes benchmark,large] [--repeats 7]
    rocprofv3 --kernel-trace --stats -d DIR/trace -o trace -- python profiles/tools/ray_query_times.py --out DIR --traced
    python profiles/tools/ray_query_times.py --out DIR --kernel-times DIR/trace      (joins the trace with DIR/plan.json)

--traced runs every call twice, each followed by a 4-byte hipMemsetAsync whose fill kernel separates the calls in the
kernel trace, and writes the order of the calls to DIR/plan.json."""
import argparse
import ctypes as C
import glob
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from vulkan_renderer_amd import capi, ray_queries as rq, renderer, synthetic  # noqa: E402

WIDTH, HEIGHT = 1920, 1080
WALKS = ("binary", "wide", "auto")
QUERIES = ("two_sided", "culled", "any")


class Device:
    def __init__(self, r):
        self.r, self.hip = r, C.CDLL("libamdhip64.so")
        self.stream = C.c_void_p(r.app.device.stream)
        self.events = [C.c_void_p(), C.c_void_p()]
        for event in self.events:
            assert self.hip.hipEventCreate(C.byref(event)) == 0
        self.marker = self.allocate(256)

    def allocate(self, nbytes):
        pointer = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(pointer), C.c_size_t(nbytes)) == 0
        return pointer

    def upload(self, array):
        array = np.ascontiguousarray(array)
        pointer = self.allocate(array.nbytes)
        assert self.hip.hipMemcpy(pointer, C.c_void_p(array.ctypes.data), C.c_size_t(array.nbytes), 1) == 0
        return pointer

    def download(self, pointer, count, dtype):
        out = np.zeros(count, dtype)
        assert self.hip.hipDeviceSynchronize() == 0
        assert self.hip.hipMemcpy(C.c_void_p(out.ctypes.data), pointer, C.c_size_t(out.nbytes), 2) == 0
        return out

    def milliseconds(self, call):
        """the time between two events around the enqueued call"""
        assert self.hip.hipEventRecord(self.events[0], self.stream) == 0
        call()
        assert self.hip.hipEventRecord(self.events[1], self.stream) == 0
        assert self.hip.hipEventSynchronize(self.events[1]) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.events[0], self.events[1]) == 0
        return float(ms.value)

    def separate(self):
        assert self.hip.hipMemsetAsync(self.marker, 0, C.c_size_t(4), self.stream) == 0


def cosine_rays(rays, hits, vertices, seed=5):
    """one cosine-distributed ray from every point that the camera rays see"""
    seen = hits["primitive"] != rq.NO_PRIMITIVE
    o, d, t = rays["origin"][seen], rays["direction"][seen], hits["t"][seen]
    v = vertices[hits["primitive"][seen]]
    normal = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    normal /= np.linalg.norm(normal, axis=-1, keepdims=True)
    normal *= -np.sign((normal * d).sum(-1, keepdims=True))
    rng = np.random.default_rng(seed)
    u0, u1 = rng.uniform(0, 1, len(o)), rng.uniform(0, 2 * np.pi, len(o))
    radius = np.sqrt(u0)
    helper = np.where(np.abs(normal[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    tangent = np.cross(normal, helper)
    tangent /= np.linalg.norm(tangent, axis=-1, keepdims=True)
    bitangent = np.cross(normal, tangent)
    direction = (radius * np.cos(u1))[:, None] * tangent + (radius * np.sin(u1))[:, None] * bitangent + np.sqrt(1 - u0)[:, None] * normal
    return rq.make_rays(o + t[:, None] * d, direction, 1.0e-3, 2.0)


def measure_scene(name, dataset, args, record, plan):
    r = renderer.Renderer()
    renderer.setup_config(r, 3, dataset, width=WIDTH, height=HEIGHT, acceleration_structure="sah_device")
    r.create_targets()
    r.create_pass()
    r.render_visibility()
    device = Device(r)
    structure = r.app.scene.acceleration_structure
    tree = {"scene": name, "triangles": int(r.app.scene.mesh.triangle_count), "leaves": int(structure.leaf_count), "wide_nodes": int(structure.wide_node_count),
            "wide_stack_need": int(structure.wide_stack_need)}
    print(tree, flush=True)
    record.append(dict(tree, kind="tree"))
    inputs = r.host_inputs()
    vertices = rq.dequantize(inputs["quantized_positions"], inputs["dequantization_factor"], inputs["dequantization_summand"])
    raster = r.pixel_rays()
    seen = r.trace_closest_hits(raster["origin"], raster["direction"], raster["t_min"], raster["t_max"], cull_back_faces=True)
    assert np.array_equal(seen["primitive"].reshape(HEIGHT, WIDTH), r.read_visibility())
    sets = {"raster": raster, "shuffled": raster[np.random.default_rng(3).permutation(len(raster))], "cosine": cosine_rays(raster, seen, vertices)}
    lib, scene, dev = r.lib, C.byref(r.app.scene), C.byref(r.app.device)

    # the door that existed before, on the same view
    def visibility():
        assert lib.render_visibility_pass(C.byref(r.app)) == 0
    if not args.traced:
        for _ in range(args.warmup):
            device.milliseconds(visibility)
        times = sorted(device.milliseconds(visibility) for _ in range(args.repeats))
        entry = {"kind": "render_visibility_pass", "scene": name, "rays": WIDTH * HEIGHT, "ms_median": times[len(times) // 2], "ms_min": times[0], "ms_max": times[-1],
                 "bytes_read_per_ray": 0, "bytes_written_per_ray": 4}
        print(entry, flush=True)
        record.append(entry)

    for set_name, rays in sets.items():
        if args.sets and set_name not in args.sets:
            continue
        count = len(rays)
        rays_pointer, out_pointer = device.upload(rays), device.allocate(16 * count)
        answers = {}
        for query in QUERIES:
            calls = {}
            for walk in WALKS:
                options = capi.RayQueryOptions(rq.WALK[walk], 0)

                def call(options=options, query=query):
                    if query == "any":
                        assert lib.trace_any_hits(scene, dev, rays_pointer, count, out_pointer, C.byref(options), None) == 0
                    else:
                        assert lib.trace_closest_hits(scene, dev, rays_pointer, count, int(query == "culled"), out_pointer, C.byref(options), None) == 0
                calls[walk] = call
            if args.traced:
                for walk, call in calls.items():
                    for _ in range(2):
                        call()
                        device.separate()
                        plan.append({"scene": name, "rays": set_name, "query": query, "walk": walk, "count": count})
                assert device.hip.hipDeviceSynchronize() == 0
                continue
            # every walk gives the answer of the binary walk
            for walk, call in calls.items():
                call()
                got = device.download(out_pointer, count * (1 if query == "any" else 16), np.uint8)
                assert np.array_equal(got, answers.setdefault(query, got)), (set_name, query, walk)
            for _ in range(args.warmup):
                for call in calls.values():
                    device.milliseconds(call)
            times = {walk: [] for walk in calls}
            for _ in range(args.repeats):
                for walk, call in calls.items():
                    times[walk].append(device.milliseconds(call))
            for walk, values in times.items():
                values.sort()
                median = values[len(values) // 2]
                entry = {"kind": "ray_query", "scene": name, "rays": set_name, "count": count, "query": query, "walk": walk, "ms_median": median, "ms_min": values[0], "ms_max": values[-1],
                         "mrays_per_s": count / median * 1.0e-3, "bytes_read_per_ray": 32, "bytes_written_per_ray": 1 if query == "any" else 16}
                print(entry, flush=True)
                record.append(entry)
        device.hip.hipFree(rays_pointer)
        device.hip.hipFree(out_pointer)
    r.close()


def kernel_times(out, trace):
    """joins the kernel trace (calls separated by fill kernels) with the plan of the traced run: kernel time per call"""
    import csv
    plan = json.load(open(os.path.join(out, "plan.json")))
    files = glob.glob(os.path.join(trace, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace below %s" % trace
    rows = sorted(csv.DictReader(open(files[0])), key=lambda row: int(row["Start_Timestamp"]))
    calls, current = [], []
    for row in rows:
        kernel = row["Kernel_Name"]
        if "k_closest_hits" in kernel or "k_any_hits" in kernel:
            current.append((kernel.split("(")[0], (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1.0e-6))
        elif "fill" in kernel.lower() and current:
            calls.append(current)
            current = []
    assert len(calls) == len(plan), (len(calls), len(plan))
    merged = {}
    for entry, kernels in zip(plan, calls):
        key = (entry["scene"], entry["rays"], entry["query"], entry["walk"])
        merged.setdefault(key, dict(entry, kind="kernel_time", calls=[]))["calls"].append(kernels)
    with open(os.path.join(out, "kernel_times.jsonl"), "w") as f:
        for entry in merged.values():
            # (the first call of the run also holds the kernels of the set-up: the call with the fewest launches counts)
            kernels = min(entry.pop("calls"), key=lambda kernels: (len(kernels), sum(ms for _, ms in kernels)))
            entry.update(kernel=kernels[-1][0], launches=len(kernels), kernel_ms=sum(ms for _, ms in kernels))
            f.write(json.dumps(entry) + "\n")
            print(entry)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", required=True)
    parser.add_argument("--scenes", default="benchmark,large")
    parser.add_argument("--sets", default="")
    parser.add_argument("--repeats", type=int, default=7)
    parser.add_argument("--warmup", type=int, default=2)
    parser.add_argument("--traced", action="store_true")
    parser.add_argument("--kernel-times", default=None)
    args = parser.parse_args()
    args.sets = [s for s in args.sets.split(",") if s]
    os.makedirs(args.out, exist_ok=True)
    if args.kernel_times:
        return kernel_times(args.out, args.kernel_times)
    record, plan = [], []
    with tempfile.TemporaryDirectory() as directory:
        for name in args.scenes.split(","):
            start = time.perf_counter()
            if name == "benchmark":
                dataset = synthetic.write_dataset(os.path.join(directory, name), grid=256, box_count=64, seed=1234, ltc_resolution=16, fresnel_count=8)
            else:
                dataset = synthetic.write_dataset(os.path.join(directory, name), seed=4321, ltc_resolution=16, fresnel_count=8, large={})
            print("%s scene written in %.1f s" % (name, time.perf_counter() - start), flush=True)
            measure_scene(name, dataset, args, record, plan)
            with open(os.path.join(args.out, "plan.json" if args.traced else "ray_query_times.jsonl"), "w") as f:
                if args.traced:
                    json.dump(plan, f)
                else:
                    f.writelines(json.dumps(entry) + "\n" for entry in record)


if __name__ == "__main__":
    main()
