"""Parity off the benchmark scene ("any scene but one"): a second dataset of 2.6 M triangles with
stacked occluders, long thin triangles, dense and sparse meshes side by side, deep occlusion and eight materials
(synthetic.make_large_scene_geometry), shaded at BASELINE sizes.

  * the libm frame of config 3 at 1920x1080 equals the reference-pinned oracle in every bit on bands of the frame
    (the oracle needs a minute per full frame of this scene on the test box; four bands are 14 % of it)
  * the three builders and both tree layouts give the same frame, bit for bit, and the same blocked rays
  * rays really leave the LDS part of the traversal stack on this scene (the slow path runs under load)
  * primary visibility equals the oracle's closest front-facing hit at 1920x1080 and 3840x2160 (both scenes)"""
import numpy as np
import pytest

import oracle
from helpers import compare
from vulkan_renderer_amd import renderer, synthetic

pytestmark = pytest.mark.gpu

BANDS = ((200, 240), (400, 440), (700, 736), (1030, 1080))


@pytest.fixture(scope="module")
def large_dataset(tmp_path_factory):
    d = tmp_path_factory.mktemp("large_dataset")
    return synthetic.write_dataset(str(d), seed=4321, ltc_resolution=32, fresnel_count=16, large={})


def render(dataset, config, width, height, builder="sah_device", binary_traversal=False, arithmetic="libm", frames_in_flight=1, **overrides):
    r = renderer.Renderer(binary_traversal=binary_traversal, frames_in_flight=frames_in_flight, arithmetic=arithmetic)
    renderer.setup_config(r, config, dataset, width=width, height=height, acceleration_structure=builder, **overrides)
    r.create_targets()
    r.create_pass()
    r.render_visibility()
    r.render()
    return r, r.read_radiance()


@pytest.fixture(scope="module")
def large_oracle(large_dataset):
    """host inputs, oracle BVH and oracle frame object of config 3 at 1920x1080 on the large scene (built once)"""
    r, image = render(large_dataset, 3, 1920, 1080, frames_in_flight=2)
    visibility = r.read_visibility()
    inputs = r.host_inputs(visibility)
    bvh = oracle.Bvh(inputs["quantized_positions"], inputs["dequantization_factor"], inputs["dequantization_summand"])
    frame = oracle.make_frame(inputs, r.oracle_settings(), bvh)
    state = {"image": image, "visibility": visibility, "inputs": inputs, "bvh": bvh, "frame": frame, "rays": r.last_ray_count(),
             "wide": r.traversal_statistics(True), "binary": r.traversal_statistics(False),
             "triangles": int(r.app.scene.mesh.triangle_count), "stack_need": int(r.app.scene.acceleration_structure.wide_stack_need),
             "build_ms": float(r.app.scene.acceleration_structure.build_milliseconds), "camera": (r.app.scene_specification.camera.near, r.app.scene_specification.camera.far)}
    r.close()
    return state


def test_large_scene_is_what_it_claims_to_be(large_oracle):
    s = large_oracle
    print({k: s[k] for k in ("triangles", "rays", "stack_need", "build_ms")}, s["wide"], s["binary"])
    assert s["triangles"] >= 2_000_000
    shaded = (s["visibility"] != 0xFFFFFFFF).mean()
    assert shaded > 0.7, shaded
    # deep occlusion: a good part of the shadow rays is blocked, and a ray walks further than in the benchmark scene
    assert 0.2 < s["wide"]["blocked_rays"] / s["wide"]["rays"] < 0.95
    assert s["wide"]["node_visits"] / s["wide"]["rays"] > 6.0
    assert s["wide"]["rays"] == s["binary"]["rays"] == s["rays"] and s["wide"]["blocked_rays"] == s["binary"]["blocked_rays"]


def test_libm_frame_of_the_large_scene_equals_the_oracle_in_every_bit(large_oracle):
    s = large_oracle
    differing, compared = 0, 0
    for y0, y1 in BANDS:
        cpu = oracle.shade(s["frame"], y0, y1)[y0:y1]
        gpu = s["image"][y0:y1]
        stats = compare(gpu, cpu)
        print((y0, y1), stats)
        differing += stats["mismatched_pixels"]
        compared += (y1 - y0) * 1920
        assert stats["nan"] == 0 and stats["bit_exact"], ((y0, y1), stats)
        # (a band that sees nothing would prove nothing)
        assert (cpu[..., :3] > 0).any(axis=-1).mean() > 0.02
    assert differing == 0 and compared >= 300_000


def test_rays_leave_the_lds_stack_on_the_large_scene(large_dataset, large_oracle, monkeypatch):
    """16 stack entries per lane live in LDS; what a ray needs beyond them spills to global memory.  The benchmark
    scene never gets there.  This one does: counted by the statistics kernel (deepest stack of any ray), and the
    frame with a 6-entry LDS part - where most rays of this scene spill - is the same frame."""
    s = large_oracle
    print("deepest stack", s["wide"]["deepest_stack"], "worst case of the build", s["stack_need"])
    assert s["stack_need"] > renderer.capi.WIDE_STACK_LDS
    monkeypatch.setenv("VKR_WIDE_STACK_LDS", "6")
    assert s["wide"]["deepest_stack"] + 1 > 6
    r, spilled = render(large_dataset, 3, 1920, 1080)
    r.close()
    assert np.array_equal(spilled.view(np.uint32), s["image"].view(np.uint32))


@pytest.mark.parametrize("refill, below, lds_stack", [(0, 166, 16), (16, 256, 16), (1, 256, 16), (24, 256, 16), (64, 256, 16), (16, 256, 6), (16, 200, 6), (16, 40, 16)])
def test_handing_rays_to_idle_lanes_changes_no_frame(large_dataset, large_oracle, monkeypatch, refill, below, lds_stack):
    """Round 5: a tracing wave that finds its batches of 64 rays less than VKR_WIDE_REFILL_BELOW / 256 busy (default 166:
    this scene's waves switch, the benchmark scene's do not) hands the next rays to lanes whose ray is done as soon as
    VKR_WIDE_REFILL lanes are idle (default 16), instead of waiting for the longest ray of every batch (VKR_WIDE_REFILL=0:
    the kernel of rounds 3 - 4; every other test of the suite runs with the defaults).  A ray query's answer does not
    depend on which lane walks it or when: the same frame and the same number of traced rays whether waves never switch,
    switch after their first batches or hand out from the start, whatever the threshold - one lane (a hand-out after
    every finished ray), a third of the wave, the whole wave - and also when most rays leave the LDS part of their stack
    while other lanes are handed new rays."""
    monkeypatch.setenv("VKR_WIDE_REFILL", str(refill))
    monkeypatch.setenv("VKR_WIDE_REFILL_BELOW", str(below))
    monkeypatch.setenv("VKR_WIDE_STACK_LDS", str(lds_stack))
    r, image = render(large_dataset, 3, 1920, 1080)
    rays = r.last_ray_count()
    r.close()
    assert rays == large_oracle["rays"]
    assert np.array_equal(image.view(np.uint32), large_oracle["image"].view(np.uint32)), int((image != large_oracle["image"]).any(axis=-1).sum())


@pytest.mark.parametrize("builder, binary_traversal", [("sah_device", True), ("lbvh_device", False), ("lbvh_device", True), ("sah_host", False)])
def test_builders_and_trees_agree_on_the_large_scene(large_dataset, large_oracle, builder, binary_traversal):
    """any-hit results do not depend on the tree: every builder and both layouts give the frame of the default
    (device SAH, four-wide), which the test above ties to the oracle"""
    r, image = render(large_dataset, 3, 1920, 1080, builder, binary_traversal)
    structure = r.app.scene.acceleration_structure
    stats = r.traversal_statistics(not binary_traversal)
    print(builder, binary_traversal, "build %.1f ms" % structure.build_milliseconds, stats)
    assert structure.builder == renderer.BVH_BUILDER[builder]
    same_visibility = np.array_equal(r.read_visibility(), large_oracle["visibility"])
    r.close()
    assert same_visibility
    assert np.array_equal(image.view(np.uint32), large_oracle["image"].view(np.uint32)), int((image != large_oracle["image"]).any(axis=-1).sum())
    # (which rays are TRACED depends on the tree since round 4: the light shafts and their occluder lists are decided by a
    # conservative walk of it - csrc/light_shafts.h - and a ray that the shading kernel decides against a list is not in
    # the queues that these statistics replay.  The frame above is what must not depend on the tree.)
    assert abs(stats["blocked_rays"] - large_oracle["wide"]["blocked_rays"]) < 0.02 * large_oracle["rays"]
    assert abs(stats["rays"] - large_oracle["rays"]) < 0.02 * large_oracle["rays"]


def test_primary_visibility_of_the_large_scene_equals_the_oracle_at_full_size(large_oracle):
    s = large_oracle
    cpu = oracle.primary_visibility(s["inputs"]["constants"], s["bvh"], 1920, 1080, *s["camera"])
    assert np.array_equal(s["visibility"], cpu), "%d pixels differ" % int((s["visibility"] != cpu).sum())


@pytest.mark.parametrize("width, height", [(1920, 1080), (3840, 2160)])
def test_primary_visibility_of_the_benchmark_scene_equals_the_oracle_at_baseline_sizes(big_dataset, width, height):
    """f1 at BASELINE sizes (until round 3 only at 320x180; every full-size test fed the oracle the GPU's own buffer)"""
    r = renderer.Renderer()
    renderer.setup_config(r, 3 if height == 1080 else 4, big_dataset, width=width, height=height, acceleration_structure="sah_device")
    r.create_targets()
    r.create_pass()
    r.render_visibility()
    gpu = r.read_visibility()
    inputs = r.host_inputs()
    cam = r.app.scene_specification.camera
    near, far = cam.near, cam.far
    r.close()
    bvh = oracle.Bvh(inputs["quantized_positions"], inputs["dequantization_factor"], inputs["dequantization_summand"])
    cpu = oracle.primary_visibility(inputs["constants"], bvh, width, height, near, far)
    assert (gpu != 0xFFFFFFFF).mean() > 0.3
    assert np.array_equal(gpu, cpu), "%d pixels differ" % int((gpu != cpu).sum())


def test_long_thin_triangles_are_split_into_several_leaves_and_nothing_else_changes(large_dataset, large_oracle, big_dataset, monkeypatch):
    """The device SAH builder cuts triangles that lie diagonally in their boxes (the slats and bars of this scene) into
    up to 16 leaves with the exact bounds of the triangle inside each slab (csrc/bvh_build.hip "fragments"): more leaves
    than triangles here, none on the benchmark scene, the same frame and the same visibility buffer either way, and far
    fewer triangle tests per ray."""
    def build(dataset, split):
        monkeypatch.setenv("VKR_BVH_SPLIT_TRIANGLES", "1" if split else "0")
        r, image = render(dataset, 3, 1920, 1080)
        structure = r.app.scene.acceleration_structure
        out = {"image": image, "visibility": r.read_visibility(), "leaves": int(structure.leaf_count), "triangles": int(r.app.scene.mesh.triangle_count),
               "nodes": int(structure.node_count), "stats": r.traversal_statistics(True)}
        r.close()
        return out
    split, whole = build(large_dataset, True), build(large_dataset, False)
    monkeypatch.delenv("VKR_BVH_SPLIT_TRIANGLES")
    print({k: split[k] for k in ("leaves", "triangles", "nodes")}, split["stats"], whole["stats"])
    assert whole["leaves"] == whole["triangles"] and whole["nodes"] == 2 * whole["triangles"] - 1
    assert split["leaves"] > split["triangles"] and split["nodes"] == 2 * split["leaves"] - 1
    assert split["leaves"] < 1.2 * split["triangles"]  # a few thousand slats and bars, not the whole mesh
    for frame in (split, whole):
        assert np.array_equal(frame["image"].view(np.uint32), large_oracle["image"].view(np.uint32))
        assert np.array_equal(frame["visibility"], large_oracle["visibility"])
    # (of the rays that were traced; a few hundred of 22 M are decided against occluder lists with one tree and traced with the other)
    assert abs(split["stats"]["blocked_rays"] - whole["stats"]["blocked_rays"]) < 0.02 * whole["stats"]["rays"]
    assert split["stats"]["triangle_tests"] < 0.5 * whole["stats"]["triangle_tests"]
    bench = build(big_dataset, True)
    assert bench["leaves"] == bench["triangles"]


def test_a_mesh_of_nothing_but_slivers_is_still_split_within_four_leaves_per_triangle(tmp_path):
    """Every triangle of this mesh wants 16 fragments (diagonal slats 6 m long, 4 cm wide): sixteenfold growth, which the
    builder refuses.  Until round 5 it then built the whole mesh unsplit; now it lowers the cap per triangle until the
    leaves fit into four per triangle.  The frame stays the oracle's either way."""
    from helpers import oracle_render
    dataset = synthetic.write_dataset(str(tmp_path / "slats"), grid=8, box_count=0, ltc_resolution=16, fresnel_count=8)
    rng = np.random.default_rng(7)
    count = 600
    centres = np.stack([rng.uniform(-4.0, 4.0, count), rng.uniform(-4.0, 4.0, count), rng.uniform(0.5, 3.0, count)], -1)
    along = np.stack([np.cos(rng.uniform(0.6, 1.0, count)), np.sin(rng.uniform(0.6, 1.0, count)), rng.uniform(-0.4, 0.4, count)], -1) * 3.0
    across = np.cross(along, np.array([0.0, 0.0, 1.0]))
    across *= 0.02 / np.linalg.norm(across, axis=-1, keepdims=True)
    a, b, c, d = centres - along - across, centres + along - across, centres + along + across, centres - along + across
    slats = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], 0)
    floor = np.array([[[-8, -8, 0], [8, -8, 0], [8, 8, 0]], [[-8, -8, 0], [8, 8, 0], [-8, 8, 0]]], np.float64)
    positions = np.concatenate([floor, slats], 0)
    normals = np.cross(positions[:, 1] - positions[:, 0], positions[:, 2] - positions[:, 0])
    normals /= np.linalg.norm(normals, axis=-1, keepdims=True)
    normals = np.repeat(normals[:, None, :], 3, 1)
    names = synthetic.write_material_textures(dataset["textures"])
    synthetic.write_vks(dataset["scene"], positions, normals, positions[:, :, :2] * 0.5, np.zeros(len(positions), np.uint8), names)
    r, image = render(dataset, 3, 384, 216)
    structure = r.app.scene.acceleration_structure
    leaves, triangles = int(structure.leaf_count), int(r.app.scene.mesh.triangle_count)
    rays = r.last_ray_count()
    cpu, _, _ = oracle_render(r, visibility=r.read_visibility(), math_mode=renderer.ORACLE_MATH_MODE[r.arithmetic])
    r.close()
    print(leaves, triangles, rays)
    assert triangles == 2 * count + 2
    assert 2 * triangles < leaves <= 4 * triangles, (leaves, triangles)
    assert rays > 0 and compare(image, cpu)["bit_exact"]
