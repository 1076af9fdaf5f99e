"""What accumulating frames on the device costs (include/vkr_frame_statistics.h): BASELINE config 3 at 1920x1080 with three
frames in flight, rendered into a ring of eight targets,
    plain      nothing else
    k1         accumulate_frames() behind every frame (one source per launch)
    k4         accumulate_frames() behind every fourth frame (four sources per launch)
the three alternately in one process, `--runs` times each; one JSON line per run and a summary line.

    python profiles/tools/accumulate_cost.py --out out/r12/accumulate_cost.jsonl
    rocprofv3 --kernel-trace --stats --output-format csv -d out/r12/trace -o t -- python profiles/tools/accumulate_cost.py --trace
    python profiles/tools/accumulate_cost.py --kernel-stats out/r12/trace --out out/r12/accumulate_kernels.jsonl

--trace runs a short k1 and k4 sequence for the profiler; --kernel-stats turns the profiler's durations of
k_accumulate_frames<K> into achieved bytes per second, pixel_count * (16 K + 96) bytes per launch."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import re
import statistics as st
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from vulkan_renderer_amd import renderer, synthetic  # noqa: E402

WIDTH, HEIGHT, RING = 1920, 1080, 8
COPY_BYTES_PER_SECOND = 6.3e12  # what a float4 copy reaches on this GPU


def run(r, ring, statistics, mode, frames):
    """Milliseconds per frame over `frames` frames, host clock around work that ends in a synchronise"""
    r.sync()
    start = time.perf_counter()
    for index in range(frames):
        r.render(ring[index % RING])
        if mode == "k1":
            statistics.accumulate([ring[index % RING]])
        elif mode == "k4" and index % 4 == 3:
            statistics.accumulate([ring[(index - 3 + k) % RING] for k in range(4)])
    if mode != "plain":
        # (the device's stream waits for the accumulations)
        statistics.resolve(ring[0], None)
    r.finish_frames()
    r.sync()
    return (time.perf_counter() - start) * 1.0e3 / frames


def kernel_stats(directory):
    lines = []
    pixels = WIDTH * HEIGHT
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            match = re.search(r"k_accumulate_frames<(\d+)>", row["Name"])
            if not match:
                continue
            k = int(match.group(1))
            average_s = float(row["AverageNs"]) * 1.0e-9
            moved = pixels * (16 * k + 96)
            lines.append({"kernel": "k_accumulate_frames<%d>" % k, "calls": int(row["Calls"]), "average_us": average_s * 1.0e6, "min_us": float(row["MinNs"]) * 1.0e-3,
                          "bytes_per_launch": moved, "achieved_TB_per_s": moved / average_s / 1.0e12, "share_of_float4_copy": moved / average_s / COPY_BYTES_PER_SECOND,
                          "us_per_frame": average_s * 1.0e6 / k})
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--kernel-stats", metavar="DIR", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = open(args.out, "w") if args.out else None

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if out:
            out.write(text + "\n")
            out.flush()
    if args.kernel_stats:
        for line in kernel_stats(args.kernel_stats):
            emit(line)
        return 0
    with tempfile.TemporaryDirectory() as directory:
        dataset = synthetic.write_dataset(directory, grid=256, box_count=64, seed=1234, ltc_resolution=64, fresnel_count=51)
        r = renderer.Renderer(frames_in_flight=3, timing_stride=1 << 30)
        renderer.setup_config(r, 3, dataset, width=WIDTH, height=HEIGHT, animate_noise=True)
        r.create_targets()
        r.create_pass()
        r.render_visibility()
        hip = C.CDLL("libamdhip64.so")
        ring = []
        for _ in range(RING):
            pointer = C.c_void_p()
            assert hip.hipMalloc(C.byref(pointer), C.c_size_t(16 * WIDTH * HEIGHT)) == 0
            ring.append(pointer.value)
        statistics = r.create_statistics()
        if args.trace:
            for mode in ("k1", "k4"):
                run(r, ring, statistics, mode, 64)
        else:
            for mode in ("plain", "k1", "k4"):
                run(r, ring, statistics, mode, args.warmup)
            results = {"plain": [], "k1": [], "k4": []}
            for index in range(args.runs):
                for mode in ("plain", "k1", "k4"):
                    ms = run(r, ring, statistics, mode, args.frames)
                    results[mode].append(ms)
                    emit({"run": index, "mode": mode, "frames": args.frames, "ms_per_frame": ms})
            plain = st.median(results["plain"])
            emit({"summary": {mode: {"median_ms_per_frame": st.median(v), "min": min(v), "max": max(v), "over_plain_ms": st.median(v) - plain} for mode, v in results.items()},
                  "workload": "config 3, %dx%d, three frames in flight, ring of %d targets, animated noise" % (WIDTH, HEIGHT, RING)})
        statistics.close()
        r.sync()
        for pointer in ring:
            hip.hipFree(C.c_void_p(pointer))
        r.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
