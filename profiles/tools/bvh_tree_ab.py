"""Are the trees of two builds of the library the same?  For the benchmark scene, the large scene and the benchmark
scene with its triangles in a random order, and for each of the three builders, both libraries build twice, every
build in a fresh process, and report the counts of the tree and what one 960x540 frame of config 3 costs to traverse
(traversal_statistics of the binary and of the four-wide tree).  The builders hand out node slots with atomics, so the
order of the nodes - and with it a few figures - may differ between two runs of ONE library: where the two runs of
library A agree, B must give exactly that; where they differ, B must lie between them or as close to one of them, in
relative terms, as they are to each other.

    python profiles/tools/bvh_tree_ab.py A.so B.so out.json        (A: the library to measure against)

The driver itself never opens the GPU and stops at the first child that fails."""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
BUILDERS = ("sah_device", "lbvh_device", "sah_host")
SCENES = {"benchmark": dict(grid=256, box_count=64, seed=1234), "large": dict(seed=4321, large={}), "shuffled": dict(grid=256, box_count=64, seed=1234, shuffle_seed=99)}
STATISTICS = ("rays", "node_visits", "triangle_tests", "blocked_rays", "longest_ray_visits", "boxes_tested", "deepest_stack", "rays_beyond_lds_stack", "node_visits_of_blocked_rays")


def build_once(dataset, builder):
    from vulkan_renderer_amd import renderer
    r = renderer.Renderer()
    renderer.setup_config(r, 3, dataset, width=960, height=540, acceleration_structure=builder)
    r.create_targets()
    r.create_pass()
    r.render_visibility()
    r.render()
    s = r.app.scene.acceleration_structure
    out = {k: int(getattr(s, k)) for k in ("node_count", "leaf_count", "wide_node_count", "wide_stack_need")}
    out["build_milliseconds"] = float(s.build_milliseconds)
    for wide in (False, True):
        statistics = r.traversal_statistics(wide)
        out.update({"%s_%s" % (statistics["tree"], k): statistics[k] for k in STATISTICS})
    r.close()
    print("RESULT " + json.dumps(out), flush=True)


def verdict(a, b):
    """a, b: the two runs per library.  Returns the fields in which A disagrees with itself and those in which B fails."""
    unstable, failed = [], []
    for field in a[0]:
        if field == "build_milliseconds":
            continue
        lo, hi = min(x[field] for x in a), max(x[field] for x in a)
        if lo != hi:
            unstable.append(field)
        slack = (hi - lo) / max(hi, 1)
        for x in b:
            if not (lo <= x[field] <= hi or min(abs(x[field] - lo), abs(x[field] - hi)) <= slack * max(hi, 1)):
                failed.append(field)
    return unstable, sorted(set(failed))


def main(library_a, library_b, out_path):
    from vulkan_renderer_amd import synthetic
    results = {}
    with tempfile.TemporaryDirectory() as directory:
        for scene, arguments in SCENES.items():
            dataset = synthetic.write_dataset(os.path.join(directory, scene), ltc_resolution=16, fresnel_count=8, **arguments)
            for builder in BUILDERS:
                runs = {"A": [], "B": []}
                for name, library in (("A", library_a), ("B", library_b), ("A", library_a), ("B", library_b)):
                    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", json.dumps(dataset), builder], env=dict(os.environ, VKR_SHADING_LIBRARY=os.path.abspath(library)),
                                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=240)
                    lines = [line for line in child.stdout.splitlines() if line.startswith("RESULT ")]
                    if child.returncode != 0 or not lines:
                        print(child.stdout[-4000:])
                        sys.exit("%s / %s with library %s ended with status %d: stopping" % (scene, builder, name, child.returncode))
                    runs[name].append(json.loads(lines[-1][7:]))
                unstable, failed = verdict(runs["A"], runs["B"])
                results["%s/%s" % (scene, builder)] = {"A": runs["A"], "B": runs["B"], "fields_in_which_A_differs_from_itself": unstable, "fields_in_which_B_is_outside_A": failed}
                print(scene, builder, "A differs from itself in", unstable, "| B outside A in", failed, flush=True)
                json.dump(results, open(out_path, "w"), indent=1)
    bad = {k: v["fields_in_which_B_is_outside_A"] for k, v in results.items() if v["fields_in_which_B_is_outside_A"]}
    print("SAME TREES" if not bad else "DIFFERENT: %s" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        build_once(json.loads(sys.argv[2]), sys.argv[3])
    else:
        sys.exit(main(*sys.argv[1:4]))
