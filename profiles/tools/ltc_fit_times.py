"""What fitting the LTC table costs (include/vkr_ltc_table.h fit_ltc_table): the default table six times with HIP events on
the device's stream around the call (kernel, read-back, quantisation, upload; the first call loads the code object), the
numpy restatement of a few chains on this host, extrapolated to the table, and smaller tables once each.

    python profiles/tools/ltc_fit_times.py [out.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d out/trace -o t -- python profiles/tools/ltc_fit_times.py"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from vulkan_renderer_amd import capi, ltc_fit, renderer  # noqa: E402

hip = C.CDLL("libamdhip64.so")
r = renderer.Renderer()
stream = C.c_void_p(r.app.device.stream)
start, stop = C.c_void_p(), C.c_void_p()
assert hip.hipEventCreate(C.byref(start)) == 0 and hip.hipEventCreate(C.byref(stop)) == 0


def timed_fit(settings):
    table = capi.LtcTable()
    r.sync()
    assert hip.hipEventRecord(start, stream) == 0
    t0 = time.perf_counter()
    assert r.lib.fit_ltc_table(C.byref(table), None, C.byref(r.app.device), C.byref(settings) if settings else None) == 0
    wall = (time.perf_counter() - t0) * 1e3
    assert hip.hipEventRecord(stop, stream) == 0 and hip.hipEventSynchronize(stop) == 0
    ms = C.c_float()
    assert hip.hipEventElapsedTime(C.byref(ms), start, stop) == 0
    r.lib.destroy_ltc_table(C.byref(table), C.byref(r.app.device))
    return ms.value, wall


out = {}
times = [timed_fit(None) for _ in range(6)]
out["default_32x32x51_n32"] = {"hip_event_ms": sorted(t[0] for t in times[1:])[2], "hip_event_ms_all": [t[0] for t in times], "call_ms_all": [t[1] for t in times]}
print("default", json.dumps(out["default_32x32x51_n32"]), flush=True)
for R, F, N in ((32, 51, 16), (32, 51, 64), (64, 51, 32), (16, 8, 32)):
    ms, wall = timed_fit(capi.LtcFitSettings(R, F, N, 200))
    out["%dx%dx%d_n%d" % (R, R, F, N)] = {"hip_event_ms": ms, "call_ms": wall}
    print(R, F, N, "%.1f ms" % ms, flush=True)
# the restatement: one process, one thread; the table has 32 * 51 chains
chains = [(2, 1), (16, 25), (31, 50)]
t0 = time.perf_counter()
ltc_fit.fit_chains(chains)
seconds = time.perf_counter() - t0
out["numpy"] = {"chains": chains, "seconds": seconds, "extrapolated_table_seconds": seconds / len(chains) * 32 * 51}
print("numpy: %d chains in %.1f s, extrapolated to the table: %.0f s" % (len(chains), seconds, out["numpy"]["extrapolated_table_seconds"]), flush=True)
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
r.close()
