"""build_milliseconds of the device SAH builder and of the LBVH on the benchmark scene (131 840 triangles) and on the large
scene (2.59 M), for two builds of the library.  A repetition is one fresh process per library - A, then B - that loads
each scene with each builder WARM_UP + TIMED times and reports the median of the timed loads; three repetitions.
The spread of A's three medians is the yardstick: B's median over all its timed builds may exceed A's by no more.

    python profiles/tools/bvh_build_times_ab.py A.so B.so out.json        (A: the library to measure against)

The driver itself never opens the GPU and stops at the first child that fails."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
WARM_UP, TIMED, REPETITIONS = 2, 10, 3
BUILDERS = ("sah_device", "lbvh_device")
SCENES = {"benchmark": dict(grid=256, box_count=64, seed=1234), "large": dict(seed=4321, large={})}


def median(values):
    return sorted(values)[len(values) // 2]


def time_builds(datasets):
    from vulkan_renderer_amd import renderer
    r = renderer.Renderer()
    out = {}
    for scene, dataset in datasets.items():
        for builder in BUILDERS:
            times = []
            for _ in range(WARM_UP + TIMED):
                r.load_scene(dataset["scene"], dataset["textures"], acceleration_structure=builder)
                times.append(float(r.app.scene.acceleration_structure.build_milliseconds))
                r.lib.destroy_scene(C.byref(r.app.scene), C.byref(r.app.device))
            out["%s/%s" % (scene, builder)] = times
    print("RESULT " + json.dumps(out), flush=True)


def main(library_a, library_b, out_path):
    from vulkan_renderer_amd import synthetic
    timed = {"A": {}, "B": {}}
    with tempfile.TemporaryDirectory() as directory:
        datasets = {scene: synthetic.write_dataset(os.path.join(directory, scene), ltc_resolution=16, fresnel_count=8, **arguments) for scene, arguments in SCENES.items()}
        for repetition in range(REPETITIONS):
            for name, library in (("A", library_a), ("B", library_b)):
                child = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", json.dumps(datasets)], env=dict(os.environ, VKR_SHADING_LIBRARY=os.path.abspath(library)),
                                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=400)
                lines = [line for line in child.stdout.splitlines() if line.startswith("RESULT ")]
                if child.returncode != 0 or not lines:
                    print(child.stdout[-4000:])
                    sys.exit("repetition %d of library %s ended with status %d: stopping" % (repetition, name, child.returncode))
                for key, times in json.loads(lines[-1][7:]).items():
                    timed[name].setdefault(key, []).append(times[WARM_UP:])
                print("repetition", repetition, name, {k: round(median(v[-1]), 3) for k, v in timed[name].items()}, flush=True)
    out, slower = {"warm_up_builds": WARM_UP, "timed_builds_per_repetition": TIMED, "repetitions": REPETITIONS}, []
    for key in timed["A"]:
        a, b = timed["A"][key], timed["B"][key]
        medians_a, medians_b = [median(v) for v in a], [median(v) for v in b]
        entry = {"A_median_ms": median(sum(a, [])), "B_median_ms": median(sum(b, [])), "A_medians_of_repetitions_ms": medians_a, "B_medians_of_repetitions_ms": medians_b,
                 "A_spread_ms": max(medians_a) - min(medians_a), "A_builds_ms": a, "B_builds_ms": b}
        entry["B_within_A_spread"] = entry["B_median_ms"] <= entry["A_median_ms"] + entry["A_spread_ms"]
        if not entry["B_within_A_spread"]:
            slower.append(key)
        out[key] = entry
        print(key, {k: (round(v, 3) if isinstance(v, float) else v) for k, v in entry.items() if not k.endswith("builds_ms")}, flush=True)
    json.dump(out, open(out_path, "w"), indent=1)
    print("NO SLOWER" if not slower else "SLOWER: %s" % slower)
    return 1 if slower else 0


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        time_builds(json.loads(sys.argv[2]))
    else:
        sys.exit(main(*sys.argv[1:4]))
