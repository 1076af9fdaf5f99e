"""What exporting a scene costs (include/vkr_scene_export.h export_scene) on the geometry of the large scene
(synthetic.make_large_scene_geometry(), 2.6 M triangles as a triangle list): three warm-up calls, then ten timed ones,
sorted and unsorted.  Per call (a) the kernels alone, between two events on the device's stream inside export_scene()
(get_scene_export_kernel_milliseconds), and (b) the whole call with allocations, upload and read-back, between two events
around it and by the host's clock.  Beside them the numpy restatement (scene_export.export) and synthetic.write_vks on
the host for the same arrays, and the bytes the kernels have to move - every array once per kernel that reads or writes
it, the sort left out - against (a).

    python profiles/tools/scene_export_times.py [out.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d out/trace -o t -- python profiles/tools/scene_export_times.py --once

--once exports a single time, sorted (what a trace wants)."""
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

WARM_UP, TIMED = 3, 10


def kernel_bytes(V, T, sort_triangles):
    """Bytes the kernels of csrc/scene_export.hip read and write without the sort's own passes"""
    boxes = 24 * V + T * (24 + 1) + (T * (36 + 12) if sort_triangles else 0)
    records = 24 * V + 16 * V
    keys = T * (12 + 8) if sort_triangles else 0
    write = T * ((8 if sort_triangles else 0) + 48 + 24 + 1 + 49)
    return boxes + records + keys + write


def median(values):
    return sorted(values)[len(values) // 2]


def main(arguments):
    from vulkan_renderer_amd import capi, renderer, scene_export, synthetic
    once = bool(arguments) and arguments[0] == "--once"
    positions, normals, uvs, materials = synthetic.make_large_scene_geometry()
    names = list(synthetic.LARGE_SCENE_MATERIALS)
    T = positions.shape[0]
    source, keepalive = scene_export.export_source(positions, normals, None, uvs, materials, names)
    V = int(source.vertex_count)
    hip = C.CDLL("libamdhip64.so")
    r = renderer.Renderer()
    stream = C.c_void_p(r.app.device.stream)
    start, stop = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(start)) == 0 and hip.hipEventCreate(C.byref(stop)) == 0
    r.lib.get_scene_export_kernel_milliseconds.restype = C.c_float
    out = {"triangles": T, "vertices": V, "warm_up_calls": WARM_UP, "timed_calls": TIMED}
    for sort_triangles in ((True,) if once else (True, False)):
        kernels, calls, wall = [], [], []
        for _ in range(1 if once else WARM_UP + TIMED):
            scene = capi.ExportedScene()
            r.sync()
            assert hip.hipEventRecord(start, stream) == 0
            t0 = time.perf_counter()
            assert r.lib.export_scene(C.byref(scene), C.byref(r.app.device), C.byref(source), int(sort_triangles)) == 0
            wall.append((time.perf_counter() - t0) * 1e3)
            assert hip.hipEventRecord(stop, stream) == 0 and hip.hipEventSynchronize(stop) == 0
            ms = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(ms), start, stop) == 0
            calls.append(ms.value)
            kernels.append(float(r.lib.get_scene_export_kernel_milliseconds()))
            r.lib.free_exported_scene(C.byref(scene))
        first = 0 if once else WARM_UP
        moved = kernel_bytes(V, T, sort_triangles)
        key = "sorted" if sort_triangles else "unsorted"
        out[key] = {"kernels_ms_median": median(kernels[first:]), "call_hip_event_ms_median": median(calls[first:]), "call_host_clock_ms_median": median(wall[first:]),
                    "kernels_ms_all": kernels, "call_hip_event_ms_all": calls, "kernel_bytes_without_sort_passes": moved,
                    "kernel_bytes_per_second": moved / (median(kernels[first:]) * 1e-3)}
        print(key, json.dumps(out[key]), flush=True)
    r.close()
    if not once:
        for sort_triangles in (True, False):
            t0 = time.perf_counter()
            scene_export.export(positions, normals, None, uvs, materials, names, sort_triangles=sort_triangles)
            out["numpy_restatement_%s_ms" % ("sorted" if sort_triangles else "unsorted")] = (time.perf_counter() - t0) * 1e3
        with tempfile.TemporaryDirectory() as directory:
            for sort_triangles in (True, False):
                t0 = time.perf_counter()
                synthetic.write_vks(os.path.join(directory, "scene.vks"), positions, normals, uvs, materials, names, sort_triangles=sort_triangles)
                out["synthetic_write_vks_%s_ms" % ("sorted" if sort_triangles else "unsorted")] = (time.perf_counter() - t0) * 1e3
        print(json.dumps({k: v for k, v in out.items() if k.endswith("_ms")}), flush=True)
        if arguments:
            json.dump(out, open(arguments[-1], "w"), indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
