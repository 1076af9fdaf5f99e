#!/usr/bin/env python3
"""What encoding a frame as JPEG on the device costs (include/vkr_jpeg.h), next to the two other ways
of getting the frame to the host: fetching the raw RGBA8 frame (begin_read_back / end_read_back) and encoding it with
the reference's writer on one host core (stbi_write_jpg of oracle/_ref, to /dev/null).

    python profiles/tools/jpeg_times.py                      # call times, both inputs, both sizes, the pipeline
    rocprofv3 --kernel-trace --stats -d OUT -- python profiles/tools/jpeg_times.py --trace     # kernel times

Call time: the host clock around begin_jpeg_encode() + end_jpeg_encode(), which ends in the wait for the slot's event,
and HIP events around the enqueued chain; the median of alternating rounds (one round visits every candidate once).
The pipeline: config 3 with three frames in flight, every frame rendered to packed RGB8, encoded on its frame stream
and fetched two frames later."""
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

from vulkan_renderer_amd import jpeg, renderer, synthetic  # noqa: E402

hip = C.CDLL("libamdhip64.so")


def device_copy(array):
    pointer = C.c_void_p()
    assert hip.hipMalloc(C.byref(pointer), C.c_size_t(array.nbytes)) == 0
    assert hip.hipMemcpy(pointer, C.c_void_p(array.ctypes.data), C.c_size_t(array.nbytes), 1) == 0
    return pointer


def median_ms(samples):
    return round(float(np.median(samples)), 4)


def reference_writer_ms(rgb, rounds):
    from oracle import reference
    if not reference.available():
        return None
    library = reference.host()
    library.stbi_write_jpg.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    rgb = np.ascontiguousarray(rgb)
    samples = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        assert library.stbi_write_jpg(b"/dev/null", rgb.shape[1], rgb.shape[0], 3, rgb.ctypes.data, 70) == 1
        samples.append((time.perf_counter() - t0) * 1e3)
    return median_ms(samples)


def measure_frame(r, rgba_pointer, width, height, rounds, variants):
    """Call times for one RGBA8 frame in device memory, per variant, and the raw read-back"""
    # (a build with a switch between kernel variants reads it from VKR_JPEG_VARIANT when an encoder is created: r19 compared
    # two coefficient kernels that way; the library itself has no switch)
    encoders = {}
    for variant in variants:
        os.environ["VKR_JPEG_VARIANT"] = variant
        encoders[variant] = r.create_jpeg_encoder(width, height, 70)
    os.environ.pop("VKR_JPEG_VARIANT", None)
    begin, end = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(begin)) == 0 and hip.hipEventCreate(C.byref(end)) == 0
    stream = C.c_void_p(r.app.device.stream)
    host = {v: [] for v in variants}
    device = {v: [] for v in variants}
    read_back = []
    size = None
    for round_index in range(rounds + 5):
        for variant in variants:
            hip.hipEventRecord(begin, stream)
            t0 = time.perf_counter()
            encoders[variant].begin(0, rgba_pointer, 4, 0)
            hip.hipEventRecord(end, stream)
            data = encoders[variant].end(0, copy=False)
            t1 = time.perf_counter()
            hip.hipEventSynchronize(end)
            elapsed = C.c_float()
            hip.hipEventElapsedTime(C.byref(elapsed), begin, end)
            size = len(data)
            if round_index >= 5:
                host[variant].append((t1 - t0) * 1e3)
                device[variant].append(elapsed.value)
        t0 = time.perf_counter()
        r.begin_read_back(0, rgba_pointer, width * height * 4)
        r.end_read_back(0, (height, width, 4), np.uint8)
        if round_index >= 5:
            read_back.append((time.perf_counter() - t0) * 1e3)
    for encoder in encoders.values():
        encoder.close()
    return {"file_bytes": size, "raw_bytes": width * height * 4, "read_back_rgba8_ms": median_ms(read_back),
            "encode_and_fetch_host_ms": {v: median_ms(host[v]) for v in variants}, "encode_chain_device_ms": {v: median_ms(device[v]) for v in variants}}


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
    encoder = r.create_jpeg_encoder(width, height, 70, slot_count=slots)
    radiance = [device_copy(np.zeros((height, width, 4), np.float32)) for _ in range(slots)]
    packed = [device_copy(np.zeros((height, width, 3), np.uint8)) for _ in range(slots)]
    sizes = []

    def run(count):
        for frame in range(count):
            slot = frame % slots
            if encode and frame >= slots:
                sizes.append(len(encoder.end(slot, copy=False)))
            stream = r.next_frame_stream()
            r.render_encoded(radiance[slot].value, packed[slot].value)
            if encode:
                encoder.begin(slot, packed[slot], 3, 0, stream=stream)
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
    for pointer in radiance + packed:
        hip.hipFree(pointer)
    return {"frames": frames, "ms_per_frame": round(seconds * 1e3 / frames, 4), "Msamples_per_s": round(width * height * samples * frames / seconds / 1e6, 1),
            "mean_file_bytes": int(np.mean(sizes)) if sizes else None}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--variants", default="", help="for an experimental build that reads VKR_JPEG_VARIANT: the variants to alternate, comma separated")
    ap.add_argument("--trace", action="store_true", help="few rounds, no host writer and no pipeline: for a run under rocprofv3 --kernel-trace")
    ap.add_argument("--out", default=None, help="also write the JSON there")
    args = ap.parse_args()
    variants = [v for v in args.variants.split(",")] if args.variants else ["library"]
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
            r.render()
            rendered = r.read_encoded()
            noise = np.random.default_rng(1).integers(0, 256, (height, width, 4), dtype=np.uint8)
            for name, image in (("config3", rendered), ("noise", noise)):
                pointer = device_copy(image)
                entry = measure_frame(r, pointer, width, height, rounds, variants)
                if not args.trace:
                    entry["reference_writer_one_core_ms"] = reference_writer_ms(image[..., :3], 3)
                    expected = jpeg.encode(image, 70)[0] if width <= 1920 else None
                    if expected is not None:
                        entry["equals_restatement"] = r.encode_jpeg(pointer, 70, width, height) == expected
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
