"""What generating a noise table costs (include/vkr_noise_table.h generate_noise_table): each default table six times
with HIP events on the device's stream around the call (allocation, kernels, read-back to the host), the numpy restatement
of the same table on this host (blue: eight of the 256 arrays, times 32), and one 128x128x4 blue table.

    python profiles/tools/noise_table_times.py [out.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d out/trace -o t -- python profiles/tools/noise_table_times.py"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from vulkan_renderer_amd import capi, renderer  # noqa: E402
from vulkan_renderer_amd import noise_tables as nt  # noqa: E402

hip = C.CDLL("libamdhip64.so")
r = renderer.Renderer()
stream = C.c_void_p(r.app.device.stream)
start, stop = C.c_void_p(), C.c_void_p()
assert hip.hipEventCreate(C.byref(start)) == 0 and hip.hipEventCreate(C.byref(stop)) == 0
out = {}
for t in ("sobol", "owen", "burley_owen", "blue"):
    res = nt.default_resolution(t)
    times, wall = [], []
    for i in range(6):
        r.lib.destroy_noise_table(C.byref(r.app.noise_table), C.byref(r.app.device))
        r.sync()
        assert hip.hipEventRecord(start, stream) == 0
        t0 = time.perf_counter()
        assert r.lib.generate_noise_table(C.byref(r.app.noise_table), C.byref(r.app.device), capi.Extent3D(*res), renderer.NOISE[t], i) == 0
        wall.append((time.perf_counter() - t0) * 1e3)
        assert hip.hipEventRecord(stop, stream) == 0 and hip.hipEventSynchronize(stop) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), start, stop) == 0
        times.append(ms.value)
    t0 = time.perf_counter()
    if t == "blue":
        for a in range(8):
            nt.blue_array(64, 64, 0, a)
        numpy_s = (time.perf_counter() - t0) * 32
    else:
        nt.sobol_table(t, 256, 64, 0)
        numpy_s = time.perf_counter() - t0
    out[t] = {"resolution": res, "hip_event_ms": sorted(times[1:])[len(times[1:]) // 2], "hip_event_ms_all": times, "call_ms_all": wall, "numpy_seconds": numpy_s}
    print(t, json.dumps(out[t]), flush=True)
# (the 1024-thread kernel with 133 KiB of LDS)
out["blue_128x128x4_call_ms"] = r.generate_noise_table("blue", (128, 128, 4), 0)
print("blue 128x128x4: %.3f ms" % out["blue_128x128x4_call_ms"])
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
r.close()
