"""What converting a texture costs (include/vkr_texture_conversion.h convert_texture): 2048x2048 and 512x512 images to
BC1 sRGB (132), BC5 (141) and RGBA16F (97), six calls each with HIP events on the device's stream around the call
(allocations, uploads, kernels, read-back to the host): the first call and the median of the other five.

    python profiles/tools/texture_conversion_times.py [out.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d out/trace -o t -- python profiles/tools/texture_conversion_times.py --once
    python profiles/tools/texture_conversion_times.py --kernels out/trace/.../t_kernel_trace.csv [out.json]

--once converts every case a single time (what a trace wants); --kernels reads a kernel trace of such a run and prints the
time of every dispatch of the converter in launch order: k_filter_level is launched per level, the highest level first.
--write DIRECTORY stores the inputs as .npy, .png and .hdr files, for timing the reference's converter on the same images."""
import ctypes as C
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

SIZES, FORMATS = (2048, 512), (132, 141, 97)


def image(size, as_float):
    """Three sinusoids and noise, seeded"""
    rng = np.random.default_rng(size)
    y, x = np.mgrid[0:size, 0:size] / float(size)
    channels = [0.5 + 0.25 * np.sin(2.0 * np.pi * (3.0 * x + 2.0 * y) + c) + 0.15 * np.sin(2.0 * np.pi * 17.0 * x - c)
                + 0.08 * np.sin(2.0 * np.pi * 41.0 * y + 2.0 * c) for c in (0.0, 1.0, 2.0, 3.0)]
    values = np.stack(channels, -1) + rng.normal(0.0, 0.03, (size, size, 4))
    return values.astype(np.float32) if as_float else np.clip(np.rint(values * 255.0), 0, 255).astype(np.uint8)


def kernels(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda row: int(row["Start_Timestamp"]))
    out = []
    for row in rows:
        name = row["Kernel_Name"].split("(")[0]
        if name.startswith("k_") and any(key in name for key in ("linearise", "filter_level", "pack_level", "encode_bc")):
            out.append({"kernel": name, "lanes": int(row.get("Grid_Size_X") or row.get("Grid_Size") or 0),
                        "microseconds": (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1.0e3})
    return out


def main(arguments):
    if arguments and arguments[0] == "--kernels":
        out = kernels(arguments[1])
        for row in out:
            print("%-18s %9d lanes %12.1f us" % (row["kernel"], row["lanes"], row["microseconds"]))
        if len(arguments) > 2:
            json.dump(out, open(arguments[2], "w"), indent=1)
        return
    if arguments and arguments[0] == "--write":
        from vulkan_renderer_amd import capi
        lib = capi.load()
        os.makedirs(arguments[1], exist_ok=True)
        for size in SIZES:
            bytes_image, float_image = np.ascontiguousarray(image(size, False)[..., :3]), np.ascontiguousarray(image(size, True)[..., :3])
            np.save(os.path.join(arguments[1], "bytes_%d.npy" % size), bytes_image)
            assert lib.write_png_rgb8(os.path.join(arguments[1], "bytes_%d.png" % size).encode(), size, size, bytes_image.ctypes.data) == 0
            assert lib.write_hdr_rgb32f(os.path.join(arguments[1], "floats_%d.hdr" % size).encode(), size, size, float_image.ctypes.data) == 0
        return
    from vulkan_renderer_amd import capi, renderer
    once = bool(arguments) and arguments[0] == "--once"
    hip = C.CDLL("libamdhip64.so")
    r = renderer.Renderer()
    stream = C.c_void_p(r.app.device.stream)
    start, stop = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(start)) == 0 and hip.hipEventCreate(C.byref(stop)) == 0
    out = {}
    for size in SIZES:
        for vk_format in FORMATS:
            pixels = image(size, vk_format == 97)
            times, wall = [], []
            for _ in range(1 if once else 6):
                texture = capi.ConvertedTexture()
                r.sync()
                assert hip.hipEventRecord(start, stream) == 0
                t0 = time.perf_counter()
                assert r.lib.convert_texture(C.byref(texture), C.byref(r.app.device), pixels.ctypes.data, size, size, 4, vk_format) == 0
                wall.append((time.perf_counter() - t0) * 1e3)
                assert hip.hipEventRecord(stop, stream) == 0 and hip.hipEventSynchronize(stop) == 0
                ms = C.c_float()
                assert hip.hipEventElapsedTime(C.byref(ms), start, stop) == 0
                times.append(ms.value)
                payload_size, levels = int(texture.payload_size), int(texture.mipmap_count)
                r.lib.free_converted_texture(C.byref(texture))
            key = "%dx%d_%d" % (size, size, vk_format)
            out[key] = {"levels": levels, "payload_bytes": payload_size, "first_call_hip_event_ms": times[0],
                        "median_of_five_hip_event_ms": sorted(times[1:])[len(times[1:]) // 2] if len(times) > 1 else None,
                        "hip_event_ms_all": times, "call_ms_all": wall}
            print(key, json.dumps(out[key]), flush=True)
    if len(arguments) > (1 if once else 0):
        json.dump(out, open(arguments[-1], "w"), indent=1)
    r.close()


if __name__ == "__main__":
    main(sys.argv[1:])
