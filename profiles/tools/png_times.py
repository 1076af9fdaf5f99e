#!/usr/bin/env python3
"""What encoding the LDR frame as a PNG file on the device costs (include/vkr_png.h), next to the two other
ways of getting its pixels to the host: fetching the RGBA8 frame (begin_read_back / end_read_back) and the PNG path of
take_screenshot(app, path, NULL), which this change leaves as it was, written to /dev/null.

    python profiles/tools/png_times.py                      # call times, two inputs, both sizes
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/tools/png_times.py --trace     # kernel times
    python profiles/tools/png_times.py --summarise-trace OUT

Inputs: the sRGB8 encoding of a rendered config-3 frame and white noise (nothing matches, every literal takes eight
bits: the worst case for the size, the best for the parse).  Call time: the host clock around begin_png_encode() +
end_png_encode(), which ends in the wait for the slot's event, and HIP events around the enqueued chain; the median of
alternating rounds (one round visits every candidate once)."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from vulkan_renderer_amd import png, renderer, synthetic  # noqa: E402

hip = C.CDLL("libamdhip64.so")
INPUT_NAMES = ("config3", "noise")
EXTENTS = ((1920, 1080), (3840, 2160))
WARM_UP = 5


def device_copy(array):
    pointer = C.c_void_p()
    assert hip.hipMalloc(C.byref(pointer), C.c_size_t(array.nbytes)) == 0
    assert hip.hipMemcpy(pointer, C.c_void_p(array.ctypes.data), C.c_size_t(array.nbytes), 1) == 0
    return pointer


def median_ms(samples):
    return round(float(np.median(samples)), 4)


def measure_frame(r, encoder, pointer, width, height, rounds, screenshot):
    """Call times for one RGBA8 frame in device memory, the raw read-back and - screenshot: for the frame in the targets -
    the host path and the device path of the *.png screenshot"""
    begin, end = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(begin)) == 0 and hip.hipEventCreate(C.byref(end)) == 0
    stream = C.c_void_p(r.app.device.stream)
    host, device, read_back, host_path, device_path = [], [], [], [], []
    size = None
    for round_index in range(rounds + WARM_UP):
        keep = round_index >= WARM_UP
        hip.hipEventRecord(begin, stream)
        t0 = time.perf_counter()
        encoder.begin(0, pointer, 4, 0)
        hip.hipEventRecord(end, stream)
        data = encoder.end(0, copy=False)
        t1 = time.perf_counter()
        hip.hipEventSynchronize(end)
        elapsed = C.c_float()
        hip.hipEventElapsedTime(C.byref(elapsed), begin, end)
        size = len(data)
        if keep:
            host.append((t1 - t0) * 1e3)
            device.append(elapsed.value)
        t0 = time.perf_counter()
        r.begin_read_back(0, pointer, width * height * 4)
        r.end_read_back(0, (height, width, 4), np.uint8)
        if keep:
            read_back.append((time.perf_counter() - t0) * 1e3)
        # (the host path takes tens of milliseconds: a fifth of the rounds)
        if screenshot and round_index % 5 == 0:
            t0 = time.perf_counter()
            assert r.lib.take_screenshot(C.byref(r.app), b"/dev/null", None) == 0
            host_path.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            assert r.lib.take_png_screenshot(C.byref(r.app), b"/dev/null") == 0
            device_path.append((time.perf_counter() - t0) * 1e3)
    entry = {"file_bytes": size, "raw_bytes": width * height * 4, "bytes_per_pixel": round(size / (width * height), 3), "read_back_rgba8_ms": median_ms(read_back),
             "encode_and_fetch_host_ms": median_ms(host), "encode_chain_device_ms": median_ms(device), "rounds": rounds}
    if screenshot:
        entry.update({"take_screenshot_host_path_ms": median_ms(host_path), "take_png_screenshot_with_encoder_creation_ms": median_ms(device_path)})
    return entry


def summarise_trace(directory, dispatches):
    """Medians per kernel and input from the *_kernel_trace.csv of a `--trace` run under rocprofv3 --kernel-trace: a chain
    begins with k_png_filter and ends with k_copy_record_out, the scans in between are the encoder's; every input is
    dispatched `dispatches` times, the inputs in the order of main(); the first WARM_UP chains of an input are left out"""
    import csv
    import glob
    paths = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    assert len(paths) == 1, paths
    with open(paths[0], newline="") as file:
        rows = sorted(csv.DictReader(file), key=lambda row: int(row["Start_Timestamp"]))
    chains, in_chain = [], False
    for row in rows:
        name = row["Kernel_Name"]
        if "k_png_filter" in name:
            chains.append({})
            in_chain = True
        if not in_chain:
            continue
        if "k_png" in name:
            short = name[name.index("k_png"):].split("(")[0].split("E")[0]
        elif "k_copy_record_out" in name:
            short = "k_copy_record_out"
        elif "scan" in name.lower():
            short = "rocprim init_lookback_scan_state" if "init" in name.lower() else "rocprim scan"
        else:
            short = "other (clears)"
        chains[-1][short] = chains[-1].get(short, 0.0) + (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3
        if "k_copy_record_out" in name:
            in_chain = False
    result = {}
    groups = [chains[i:i + dispatches] for i in range(0, len(chains), dispatches)]
    for n, group in enumerate(groups):
        width, height = EXTENTS[n // len(INPUT_NAMES)] if n // len(INPUT_NAMES) < len(EXTENTS) else (0, 0)
        kept = group[WARM_UP:]
        entry = {kernel: {"median_us": round(float(np.median([chain.get(kernel, 0.0) for chain in kept])), 2)} for kernel in kept[0]}
        entry["sum_of_medians_us"] = round(sum(k["median_us"] for k in entry.values()), 2)
        entry["chains"] = len(kept)
        result["%s_%dx%d" % (INPUT_NAMES[n % len(INPUT_NAMES)], width, height)] = entry
    return result


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--trace", action="store_true", help="eleven kept dispatches per input and no host path: for a run under rocprofv3 --kernel-trace")
    ap.add_argument("--out", default=None, help="also write the JSON there")
    ap.add_argument("--summarise-trace", metavar="DIR", default=None, help="no measurement: the medians per kernel and input from the kernel trace of a --trace run in DIR")
    args = ap.parse_args()
    rounds = 11 if args.trace else args.rounds
    if args.summarise_trace:
        result = summarise_trace(args.summarise_trace, 11 + WARM_UP)
        print(json.dumps(result, indent=1))
        if args.out:
            with open(args.out, "w") as file:
                json.dump(result, file, indent=1)
        return
    result = {"frames": {}}
    with tempfile.TemporaryDirectory() as tmp:
        dataset = synthetic.write_dataset(tmp, grid=256, box_count=64, seed=1234, ltc_resolution=64, fresnel_count=51)
        for width, height in EXTENTS:
            r = renderer.Renderer()
            renderer.setup_config(r, 3, dataset, width=width, height=height)
            r.create_targets()
            r.create_pass()
            r.render_visibility()
            r.render()
            # the sRGB8 encoding of the frame stays in the encoded target
            frame = r.read_encoded()
            r.sync()
            noise = np.random.default_rng(1).integers(0, 256, (height, width, 4), dtype=np.uint8)
            encoder = r.create_png_encoder(width, height)
            inputs = (("config3", C.c_void_p(r.app.render_targets.encoded), False, frame), ("noise", device_copy(noise), True, noise))
            for name, pointer, owned, image in inputs:
                entry = measure_frame(r, encoder, pointer, width, height, rounds, screenshot=name == "config3" and not args.trace)
                if not args.trace and width <= 1920:
                    entry["equals_restatement"] = encoder.encode(pointer) == png.encode(image)
                if owned:
                    hip.hipFree(pointer)
                result["frames"]["%s_%dx%d" % (name, width, height)] = entry
                print(name, width, height, json.dumps(entry), flush=True)
            r.close()
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as file:
            json.dump(result, file, indent=1)


if __name__ == "__main__":
    main()
