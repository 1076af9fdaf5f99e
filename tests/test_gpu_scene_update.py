"""Moving geometry on the device (include/vkr_scene_update.h, csrc/bvh_refit.hip): a refitted tree is the tree of the
numpy restatement in every byte, answers ray queries like the brute force, shades the oracle's frame, and takes nothing
of the tree before it along in the caches of the shading pass.  Meshes and motions: scene_update_cases.py."""
import ctypes as C

import numpy as np
import pytest

import oracle
import scene_update_cases as cases
from helpers import compare, oracle_render
from vulkan_renderer_amd import capi, ray_queries, renderer, scene_update

pytestmark = pytest.mark.gpu

BUILDERS = cases.BUILDERS
SMALL = [1, 2, 3, 17, "slats"]
RESTING, KEPT_KINDS = 21, (1, 2, 16, 17)  # (the kinds of verdict words: test_gpu_light_shaft_reuse.py)


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    """one dataset per mesh, written once"""
    return {name: cases.write_case(tmp_path_factory.mktemp("update_%s" % name), name) for name in cases.MESHES}


@pytest.fixture(scope="module")
def expected_frames():
    """the oracle's visibility and frame per (mesh, step): the same for every builder"""
    return {}


def start(dataset, builder, scene_path=None, create_pass=True):
    r = renderer.Renderer()
    renderer.setup_config(r, 3, dict(dataset, scene=scene_path or dataset["scene"]), width=cases.WIDTH, height=cases.HEIGHT, acceleration_structure=builder)
    if create_pass:
        r.create_targets()
        r.create_pass()
    return r


def constants_of(r):
    mesh = r.app.scene.mesh
    return np.array(mesh.dequantization_factor[:], np.float32), np.array(mesh.dequantization_summand[:], np.float32)


def host_words(r):
    mesh = r.app.scene.mesh
    return np.ctypeslib.as_array(mesh.host_positions, (3 * mesh.triangle_count, 2)).copy()


def render_frame(r):
    r.render_visibility()
    r.render()
    return r.read_visibility(), r.read_radiance()


def oracle_frame(r, expected_frames, key):
    """-> (visibility, frame) of the oracle for the mesh that r holds now"""
    if key not in expected_frames:
        cam = r.app.scene_specification.camera
        cpu, inputs, bvh = oracle_render(r, math_mode=renderer.ORACLE_MATH_MODE[r.arithmetic])
        expected_frames[key] = (oracle.primary_visibility(inputs["constants"], bvh, cases.WIDTH, cases.HEIGHT, cam.near, cam.far), cpu)
    return expected_frames[key]


def assert_oracle_frame(r, expected_frames, key):
    visibility, image = render_frame(r)
    cpu_visibility, cpu = oracle_frame(r, expected_frames, key)
    assert np.array_equal(visibility, cpu_visibility), "%d pixels see another triangle" % int((visibility != cpu_visibility).sum())
    assert compare(image, cpu)["bit_exact"], compare(image, cpu)
    return visibility, image


class DeviceArray:
    """a copy of a host array in device memory"""

    def __init__(self, array):
        self.hip = renderer._hip_runtime()
        self.pointer = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.pointer), array.nbytes) == 0
        assert self.hip.hipMemcpy(self.pointer, array.ctypes.data, array.nbytes, 1) == 0

    def free(self):
        self.hip.hipFree(self.pointer)


@pytest.mark.parametrize("name", SMALL, ids=str)
@pytest.mark.parametrize("builder", BUILDERS)
def test_identity_and_restatement(datasets, builder, name):
    """An update with the scene's own positions reproduces the build byte for byte - the builders' inner boxes are the exact
    unions of their primitives' boxes, padded monotonically, and quantisation is monotone - and an update with moved ones
    gives the bytes of refit_reference(), from host memory and from device memory alike."""
    r = start(datasets[name], builder, create_pass=False)
    try:
        factor, summand = constants_of(r)
        built, rest = r.read_acceleration_structure(), host_words(r)
        triangles = int(r.app.scene.mesh.triangle_count)
        print(name, builder, {k: built[k] for k in ("node_count", "leaf_count", "wide_node_count", "build_serial")})
        assert built["leaf_fragments"].shape == (built["leaf_count"],)
        counts, slabs = built["leaf_fragments"] & 0xFFFF, built["leaf_fragments"] >> 16
        assert (counts >= 1).all() and (counts <= 16).all() and (slabs < counts).all()
        if builder == "sah_device" and name == "slats":
            # the fragment path must not drop out of this test unnoticed
            assert built["leaf_count"] > triangles and (counts > 1).sum() > 100 and len(np.unique(counts)) > 2
        elif builder != "sah_device":
            # (the device SAH builder may split a sliver of any mesh: three of the small triangles of mesh 17)
            assert built["leaf_count"] == triangles and (counts == 1).all()
        assert built["leaf_count"] == triangles + int((counts > 1).sum()) - len(np.unique(built["triangle_vertices"][0::3, 3].view(np.uint32)[counts > 1]))
        report = r.update_geometry(rest)
        same = r.read_acceleration_structure()
        assert scene_update.differences(same, built) == []
        assert not report["rebuilt"] and report["build_serial"] == same["build_serial"] > built["build_serial"] and report["milliseconds"] > 0.0
        assert np.array_equal(same["leaf_fragments"], built["leaf_fragments"])
        assert scene_update.differences(same, scene_update.refit_reference(built, rest, factor, summand)) == []
        # moved, from host memory
        moved = cases.quantized(datasets[name], cases.motion(name, 1))
        r.update_geometry(moved)
        after = r.read_acceleration_structure()
        assert scene_update.differences(after, built) != []
        assert scene_update.differences(after, scene_update.refit_reference(built, moved, factor, summand)) == []
        assert np.array_equal(host_words(r), moved)
        # moved further, from device memory
        further = cases.quantized(datasets[name], cases.motion(name, 2 if name != "occluder" else 3))
        on_device = DeviceArray(further)
        try:
            r.update_geometry(on_device.pointer, on_device=True)
        finally:
            on_device.free()
        after = r.read_acceleration_structure()
        assert scene_update.differences(after, scene_update.refit_reference(built, further, factor, summand)) == []
        assert np.array_equal(host_words(r), further)
    finally:
        r.close()


RAY_ANSWERS = {}


@pytest.mark.parametrize("name", SMALL, ids=str)
@pytest.mark.parametrize("builder", BUILDERS)
def test_ray_queries_after_a_motion(datasets, builder, name):
    """4096 rays against the moved vertices: closest hit, two-sided and culled, and any hit equal the brute force in every
    bit, on the binary walk, the wide walk and the wide walk with two stack entries in LDS"""
    r = start(datasets[name], builder, create_pass=False)
    try:
        factor, summand = constants_of(r)
        moved = cases.quantized(datasets[name], cases.motion(name, 1))
        r.update_geometry(moved)
        if name not in RAY_ANSWERS:
            vertices = ray_queries.dequantize(moved, factor, summand)
            rays = ray_queries.test_rays(vertices, 4096, 29)
            RAY_ANSWERS[name] = (rays, ray_queries.closest_hits_brute_force(vertices, rays, False), ray_queries.closest_hits_brute_force(vertices, rays, True), ray_queries.any_hits_brute_force(vertices, rays))
        rays, two_sided, culled, blocked = RAY_ANSWERS[name]
        assert (two_sided["primitive"] != ray_queries.NO_PRIMITIVE).mean() > 0.2
        walks = [("binary", 0)] + ([("wide", 0), ("wide", 2)] if r.app.scene.acceleration_structure.wide_nodes else [])
        assert len(walks) == (1 if name == 1 else 3)
        arguments = (rays["origin"], rays["direction"], rays["t_min"], rays["t_max"])
        for walk, lds in walks:
            for cull, expected in ((False, two_sided), (True, culled)):
                got = r.trace_closest_hits(*arguments, cull_back_faces=cull, walk=walk, lds_stack_entries=lds)
                wrong = np.nonzero(got.view(np.uint32).reshape(-1, 4) != expected.view(np.uint32).reshape(-1, 4))[0]
                assert len(wrong) == 0, (walk, lds, cull, len(wrong), got[wrong[:3]], expected[wrong[:3]])
            assert np.array_equal(r.trace_any_hits(*arguments, walk=walk, lds_stack_entries=lds), blocked), (walk, lds)
    finally:
        r.close()


@pytest.mark.parametrize("name", SMALL, ids=str)
@pytest.mark.parametrize("builder", BUILDERS)
def test_frames_after_a_motion(datasets, expected_frames, tmp_path, builder, name):
    """update, render_visibility, render: the visibility buffer and the frame of the oracle for the moved mesh, and of a
    renderer that loads the moved mesh from a file"""
    dataset = datasets[name]
    r = start(dataset, builder)
    try:
        render_frame(r)
        moved = cases.quantized(dataset, cases.motion(name, 1))
        r.update_geometry(moved)
        visibility, image = assert_oracle_frame(r, expected_frames, (name, 1))
    finally:
        r.close()
    target = str(tmp_path / "moved.vks")
    cases.rewrite_vks_positions(dataset["scene"], target, moved)
    fresh = start(dataset, builder, scene_path=target)
    try:
        fresh_visibility, fresh_image = render_frame(fresh)
    finally:
        fresh.close()
    assert np.array_equal(visibility, fresh_visibility) and compare(image, fresh_image)["bit_exact"]


@pytest.mark.parametrize("builder", BUILDERS)
def test_nothing_of_the_old_tree_is_kept(datasets, expected_frames, builder):
    """Frames that stand still let the shaft verdicts rest and store the prepared polygons; then an occluder moves out of
    the shaft of the first light.  The frame after the update is the oracle's for the new mesh, and the statistics show a
    launch that kept nothing."""
    r = start(datasets["occluder"], builder)
    try:
        r.render_visibility()
        for _ in range(3):
            r.render()
            before = r.read_radiance()
        prepared, shafts, words = r.prepared_polygon_statistics(), r.light_shaft_statistics(), r.light_shaft_words()
        print(builder, prepared, shafts)
        assert prepared["mode"] == "loading" and prepared["state"] == "valid" and prepared["launches"] == {"plain": 1, "storing": 1, "loading": 1}
        assert words.size and np.isin(words & 0xFF, KEPT_KINDS + (RESTING,)).any()
        _, oracle_before = oracle_frame(r, expected_frames, ("occluder", 0))
        assert compare(before, oracle_before)["bit_exact"]
        r.update_geometry(cases.quantized(datasets["occluder"], cases.motion("occluder", 1)))
        _, image = assert_oracle_frame(r, expected_frames, ("occluder", 1))
        _, oracle_after = expected_frames[("occluder", 1)]
        # the oracle alone says that the motion shows: in a hundredth of the pixels at least
        assert (oracle_before.view(np.uint32) != oracle_after.view(np.uint32)).any(axis=-1).mean() >= 0.01
        assert (before.view(np.uint32) != image.view(np.uint32)).any(axis=-1).mean() >= 0.01
        prepared, words = r.prepared_polygon_statistics(), r.light_shaft_words()
        print(prepared, r.light_shaft_statistics())
        assert prepared["mode"] == "plain" and prepared["state"] == "empty" and prepared["launches"] == {"plain": 2, "storing": 1, "loading": 1}
        assert words.size and not ((words & 0xFF) == RESTING).any()
    finally:
        r.close()


@pytest.mark.parametrize("builder", BUILDERS)
def test_policies_and_report(datasets, expected_frames, builder):
    dataset = datasets[17]
    r = start(dataset, builder)
    try:
        factor, summand = constants_of(r)
        built, rest = r.read_acceleration_structure(), host_words(r)
        # the cost of the tree as built, taken by the first update; an update that moves nothing costs the same
        report = r.update_geometry(rest, measure_cost=True)
        sums, cost = scene_update.tree_cost(built["nodes"], built["grid_inverse_cell"])
        assert report["cost"] == report["built_cost"] == cost > 0.0 and not report["rebuilt"]
        moved = cases.quantized(dataset, cases.motion(17, 3))
        report = r.update_geometry(moved, measure_cost=True)
        expected = scene_update.refit_reference(built, moved, factor, summand)
        assert report["cost"] == expected["cost"] and report["built_cost"] == cost and expected["cost_sums"] != sums
        # without measure_cost the report says nothing about it
        silent = r.update_geometry(moved)
        assert silent["cost"] == 0.0 and silent["built_cost"] == 0.0
        ratio = report["cost"] / report["built_cost"]
        print(builder, "cost ratio after the motion: %.4f" % ratio)
        kept = r.update_geometry(moved, policy="auto", rebuild_above=ratio * 1.001)
        assert not kept["rebuilt"] and kept["cost"] == report["cost"]
        never = r.update_geometry(moved, policy="auto", rebuild_above=0.0)
        assert not never["rebuilt"]
        serial = never["build_serial"]
        rebuilt = r.update_geometry(moved, policy="auto", rebuild_above=ratio * 0.999)
        assert rebuilt["rebuilt"] and rebuilt["build_serial"] > serial and rebuilt["cost"] == report["cost"]
        fresh = r.read_acceleration_structure()
        assert fresh["builder"] == renderer.BVH_BUILDER[builder] and fresh["node_count"] == built["node_count"]
        # the next update takes the cost of the new tree as built
        again = r.update_geometry(moved, measure_cost=True)
        assert again["built_cost"] == again["cost"] == scene_update.tree_cost(fresh["nodes"], fresh["grid_inverse_cell"])[1]
        # the rebuild policy, and the frame of the tree it leaves
        step = cases.quantized(dataset, cases.motion(17, 1))
        report = r.update_geometry(step, policy="rebuild")
        assert report["rebuilt"] and report["build_serial"] > again["build_serial"] and report["milliseconds"] > 0.0
        assert_oracle_frame(r, expected_frames, (17, 1))
    finally:
        r.close()


@pytest.mark.parametrize("builder", BUILDERS)
def test_failures_leave_the_scene_as_it_was(datasets, builder):
    r = start(datasets[17], builder, create_pass=False)
    try:
        before, words = r.read_acceleration_structure(), host_words(r)
        scene, device, report = C.byref(r.app.scene), C.byref(r.app.device), capi.SceneUpdateReport()
        call = r.lib.update_scene_geometry
        assert call(None, device, words.ctypes.data, None, None, C.byref(report)) == 1
        assert call(scene, None, words.ctypes.data, None, None, C.byref(report)) == 1
        assert call(scene, device, None, None, None, C.byref(report)) == 1
        for options in (capi.SceneUpdateOptions(3, 0, 1, 0, 0.0), capi.SceneUpdateOptions(0xFFFFFFFF, 0, 1, 0, 0.0), capi.SceneUpdateOptions(2, 0, 1, 0, -0.5),
                        capi.SceneUpdateOptions(0, 0, 1, 0, float("nan")), capi.SceneUpdateOptions(1, 0, 1, 1, -float("inf"))):
            assert call(scene, device, words.ctypes.data, None, C.byref(options), C.byref(report)) == 1
        with pytest.raises(ValueError):
            r.update_geometry(words[:-1])
        after = r.read_acceleration_structure()
        assert after["build_serial"] == before["build_serial"] == int(r.app.scene.acceleration_structure.build_serial)
        assert np.array_equal(after["nodes"][[0, -1]], before["nodes"][[0, -1]]) and scene_update.differences(after, before) == []
        # a scene without acceleration structure gets the uploads and nothing else
        bare = renderer.Renderer()
        try:
            bare.load_scene(datasets[17]["scene"], datasets[17]["textures"], acceleration_structure=False)
            moved = cases.quantized(datasets[17], cases.motion(17, 1))
            report = bare.update_geometry(moved)
            assert report == {"rebuilt": False, "build_serial": 0, "milliseconds": report["milliseconds"], "cost": 0.0, "built_cost": 0.0}
            assert np.array_equal(host_words(bare), moved) and not bare.app.scene.acceleration_structure.nodes
        finally:
            bare.close()
    finally:
        r.close()


@pytest.mark.parametrize("name", [17, "slats"], ids=str)
@pytest.mark.parametrize("builder", BUILDERS)
def test_twenty_updates_in_a_row(datasets, expected_frames, builder, name):
    """counters that an update did not leave as it found them would show in the next one"""
    dataset = datasets[name]
    r = start(dataset, builder)
    try:
        factor, summand = constants_of(r)
        built = r.read_acceleration_structure()
        serial = built["build_serial"]
        for step in range(1, 21):
            words = cases.quantized(dataset, cases.motion(name, step))
            report = r.update_geometry(words, measure_cost=step % 4 == 0)
            assert report["build_serial"] > serial
            serial = report["build_serial"]
        assert scene_update.differences(r.read_acceleration_structure(), scene_update.refit_reference(built, words, factor, summand)) == []
        assert_oracle_frame(r, expected_frames, (name, 20))
    finally:
        r.close()


def test_the_command_line_renders_a_sequence(datasets, tmp_path, capsys):
    """python -m vulkan_renderer_amd.scene_update: one PNG per frame of the wobbling mesh, and with --time a line per frame"""
    import os
    out = tmp_path / "frames"
    assert scene_update.main([os.path.dirname(datasets[17]["scene"]), "--frames", "3", "--amplitude", "0.2", "--out", str(out), "--width", "64", "--height", "36",
                              "--policy", "auto", "--rebuild-above", "2", "--time"]) == 0
    files = sorted(os.listdir(out))
    assert files == ["frame_0000.png", "frame_0001.png", "frame_0002.png"]
    images = [open(out / name, "rb").read() for name in files]
    assert all(image[:8] == b"\x89PNG\r\n\x1a\n" and image[16:24] == (64).to_bytes(4, "big") + (36).to_bytes(4, "big") for image in images)
    assert images[0] != images[1] != images[2]
    lines = [line for line in capsys.readouterr().out.splitlines() if line.startswith("frame ")]
    assert len(lines) == 3 and all("cost ratio" in line and "a rebuild" in line for line in lines)
