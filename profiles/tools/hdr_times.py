#!/usr/bin/env python3
"""What encoding a float frame as a Radiance file on the device costs (include/vkr_hdr.h), next to the two
other ways of getting its values to the host: fetching the RGBA32F frame (begin_read_back / end_read_back) and the host
path of take_screenshot(app, NULL, path), written to /dev/null.

    python profiles/tools/hdr_times.py                      # call times, four inputs, both sizes, the pipeline
    rocprofv3 --kernel-trace --stats -d OUT -- python profiles/tools/hdr_times.py --trace     # kernel times

Inputs: a rendered config-3 frame, the mean of 64 such frames with animated noise, white noise in [0, 1) and white noise
over many decades (nothing repeats in any plane: the worst case).  Call time: the host clock around begin_hdr_encode() +
end_hdr_encode(), which ends in the wait for the slot's event, and HIP events around the enqueued chain; the median of
alternating rounds (one round visits every candidate once).  The pipeline: config 3 with three frames in flight, every
frame encoded on its frame stream and fetched two frames later."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from vulkan_renderer_amd import hdr, renderer, synthetic  # noqa: E402

hip = C.CDLL("libamdhip64.so")


def device_copy(array):
    pointer = C.c_void_p()
    assert hip.hipMalloc(C.byref(pointer), C.c_size_t(array.nbytes)) == 0
    assert hip.hipMemcpy(pointer, C.c_void_p(array.ctypes.data), C.c_size_t(array.nbytes), 1) == 0
    return pointer


def median_ms(samples):
    return round(float(np.median(samples)), 4)


def measure_frame(r, encoder, pointer, width, height, rounds, screenshot):
    """Call times for one RGBA32F frame in device memory, the raw read-back and - screenshot: for the frame in the radiance
    target - the host path and the device path of the *.hdr screenshot"""
    begin, end = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(begin)) == 0 and hip.hipEventCreate(C.byref(end)) == 0
    stream = C.c_void_p(r.app.device.stream)
    host, device, read_back, host_path, device_path = [], [], [], [], []
    size = None
    for round_index in range(rounds + 5):
        keep = round_index >= 5
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
        r.begin_read_back(0, pointer, width * height * 16)
        r.end_read_back(0, (height, width, 4), np.float32)
        if keep:
            read_back.append((time.perf_counter() - t0) * 1e3)
        # (the host path takes tens of milliseconds: a fifth of the rounds)
        if screenshot and round_index % 5 == 0:
            t0 = time.perf_counter()
            assert r.lib.take_screenshot(C.byref(r.app), None, b"/dev/null") == 0
            host_path.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            assert r.lib.take_hdr_screenshot(C.byref(r.app), b"/dev/null") == 0
            device_path.append((time.perf_counter() - t0) * 1e3)
    entry = {"file_bytes": size, "raw_bytes": width * height * 16, "bytes_per_pixel": round(size / (width * height), 3), "read_back_rgba32f_ms": median_ms(read_back),
             "encode_and_fetch_host_ms": median_ms(host), "encode_chain_device_ms": median_ms(device)}
    if screenshot:
        entry.update({"take_screenshot_host_path_ms": median_ms(host_path), "take_hdr_screenshot_with_encoder_creation_ms": median_ms(device_path)})
    return entry


def pipeline(dataset, frames, encode):
    """config 3, three frames in flight; with encode every frame is encoded on its frame stream and fetched two frames later"""
    r = renderer.Renderer(frames_in_flight=3)
    renderer.setup_config(r, 3, dataset)
    r.create_targets()
    r.create_pass()
    r.render_visibility()
    e = r.app.swapchain.extent
    width, height, samples = e.width, e.height, r.app.render_settings.sample_count
    slots = 3
    encoder = r.create_hdr_encoder(width, height, slot_count=slots)
    radiance = [device_copy(np.zeros((height, width, 4), np.float32)) for _ in range(slots)]
    sizes = []

    def run(count):
        for frame in range(count):
            slot = frame % slots
            if encode and frame >= slots:
                sizes.append(len(encoder.end(slot, copy=False)))
            stream = r.next_frame_stream()
            r.render(radiance[slot].value)
            if encode:
                encoder.begin(slot, radiance[slot], 4, 0, stream=stream)
        if encode:
            for slot in range(min(slots, count)):
                encoder.end(slot, copy=False)
        r.finish_frames()
        r.sync()

    run(60)
    t0 = time.perf_counter()
    run(frames)
    seconds = time.perf_counter() - t0
    r.close()
    for pointer in radiance:
        hip.hipFree(pointer)
    return {"frames": frames, "ms_per_frame": round(seconds * 1e3 / frames, 4), "Msamples_per_s": round(width * height * samples * frames / seconds / 1e6, 1),
            "mean_file_bytes": int(np.mean(sizes)) if sizes else None}


INPUT_NAMES = ("config3", "config3_mean_of_64", "noise", "noise_over_40_decades")


def summarise_trace(directory, dispatches=11):
    """Medians per kernel and input from the *_kernel_trace.csv of a `--trace` run under rocprofv3 --kernel-trace: the
    encoder's kernels are dispatched `dispatches` times per input, the inputs in the order of main()"""
    import csv
    import glob
    paths = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    assert len(paths) == 1, paths
    durations = {}
    with open(paths[0], newline="") as file:
        rows = sorted(csv.DictReader(file), key=lambda row: int(row["Start_Timestamp"]))
    in_chain = False
    for row in rows:
        name = row["Kernel_Name"]
        # (the scan's kernels count between the two passes over the rows only: other units scan too)
        # (the copy-out is the kernel that the encoders share, csrc/output_slots.hip: in this run every one is an HDR file's)
        own = "k_hdr" if "k_hdr" in name else "k_copy_record_out" if "k_copy_record_out" in name else None
        in_chain = "k_hdr_row_sizes" in name or (in_chain and not own)
        if own or (in_chain and "scan" in name.lower()):
            short = name[name.index(own):].split("(")[0].split("E")[0] if own else ("rocprim init_lookback_scan_state" if "init" in name.lower() else "rocprim scan")
            durations.setdefault(short, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3)
    result = {}
    for kernel, values in durations.items():
        groups = [values[i:i + dispatches] for i in range(0, len(values), dispatches)]
        for n, group in enumerate(groups):
            extent = "1920x1080" if n < len(INPUT_NAMES) else "3840x2160"
            result.setdefault("%s_%s" % (INPUT_NAMES[n % len(INPUT_NAMES)], extent), {})[kernel] = {"median_us": round(float(np.median(group)), 2), "dispatches": len(group)}
    for entry in result.values():
        entry["sum_of_medians_us"] = round(sum(k["median_us"] for k in entry.values()), 2)
    return result


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--trace", action="store_true", help="eleven dispatches per input, no host path and no pipeline: for a run under rocprofv3 --kernel-trace")
    ap.add_argument("--out", default=None, help="also write the JSON there")
    ap.add_argument("--summarise-trace", metavar="DIR", default=None, help="no measurement: the medians per kernel and input from the kernel trace of a --trace run in DIR")
    args = ap.parse_args()
    if args.summarise_trace:
        result = summarise_trace(args.summarise_trace)
        print(json.dumps(result, indent=1))
        if args.out:
            with open(args.out, "w") as file:
                json.dump(result, file, indent=1)
        return
    rounds = 6 if args.trace else args.rounds
    result = {"frames": {}}
    with tempfile.TemporaryDirectory() as tmp:
        dataset = synthetic.write_dataset(tmp, grid=256, box_count=64, seed=1234, ltc_resolution=64, fresnel_count=51)
        for width, height in ((1920, 1080), (3840, 2160)):
            r = renderer.Renderer()
            renderer.setup_config(r, 3, dataset, width=width, height=height)
            r.create_targets()
            r.create_pass()
            r.render_visibility()
            # the mean of 64 frames with animated noise, then the frame itself, which stays in the radiance target
            mean_pointer = device_copy(np.zeros((height, width, 4), np.float32))
            animate_before = r.app.render_settings.animate_noise
            r.app.render_settings.animate_noise = 1
            statistics = r.create_statistics()
            for _ in range(64):
                r.render()
                statistics.accumulate()
            statistics.resolve(mean_pointer, None)
            r.sync()
            statistics.close()
            r.app.render_settings.animate_noise = animate_before
            r.render()
            r.sync()
            rng = np.random.default_rng(1)
            noise = rng.random((height, width, 4), np.float32)
            decades = (noise * 10.0 ** rng.integers(-20, 20, (height, width, 1))).astype(np.float32)
            encoder = r.create_hdr_encoder(width, height)
            inputs = (("config3", C.c_void_p(r.app.render_targets.radiance), False), ("config3_mean_of_64", mean_pointer, True),
                      ("noise", device_copy(noise), True), ("noise_over_40_decades", device_copy(decades), True))
            for name, pointer, owned in inputs:
                entry = measure_frame(r, encoder, pointer, width, height, rounds, screenshot=name == "config3" and not args.trace)
                if not args.trace and width <= 1920:
                    image = np.zeros((height, width, 4), np.float32)
                    assert hip.hipMemcpy(C.c_void_p(image.ctypes.data), pointer, C.c_size_t(image.nbytes), 2) == 0
                    entry["equals_restatement"] = encoder.encode(pointer) == hdr.encode(image)
                if owned:
                    hip.hipFree(pointer)
                result["frames"]["%s_%dx%d" % (name, width, height)] = entry
                print(name, width, height, json.dumps(entry), flush=True)
            r.close()
        if not args.trace:
            for round_index in range(3):
                for name, encode in (("render_only", False), ("render_encode_fetch", True)):
                    entry = pipeline(dataset, args.frames, encode)
                    result.setdefault("pipeline_config3_3_frames_in_flight", {}).setdefault(name, []).append(entry)
                    print(name, json.dumps(entry), flush=True)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as file:
            json.dump(result, file, indent=1)


if __name__ == "__main__":
    main()
