"""The BVH builders on meshes of 1, 2, 3 and 17 triangles (csrc/bvh_build.hip): the ends of the host control flow that
the scenes of the other tests never reach - a tree that is a single leaf (no level of the SAH build, no inner node of
the radix tree, no collapse), level loops that run once, and 17 triangles, which cross no power of two and give the
collapse more than one level.  Each tree must shade the oracle's frame and see the oracle's triangles."""
import numpy as np
import pytest

import oracle
from helpers import compare, oracle_render
from vulkan_renderer_amd import renderer, synthetic

pytestmark = pytest.mark.gpu

WIDTH, HEIGHT = 64, 36
BUILDERS = ("sah_device", "lbvh_device", "sah_host")
# the floor: one triangle that reaches from the camera to beyond the lights of config 3, and the quad of the other tests
FLOOR_TRIANGLE = [[[-8, -8, 0], [24, -8, 0], [-8, 24, 0]]]
FLOOR_QUAD = [[[-8, -8, 0], [8, -8, 0], [8, 8, 0]], [[-8, -8, 0], [8, 8, 0], [-8, 8, 0]]]


def small_triangles(count, seed=17):
    """triangles about 0.4 m across between the floor and the lights, in front of the camera"""
    rng = np.random.default_rng(seed)
    centres = np.stack([rng.uniform(-2.5, 2.5, count), rng.uniform(0.0, 5.0, count), rng.uniform(0.4, 1.8, count)], -1)
    return centres[:, None, :] + rng.uniform(-0.2, 0.2, (count, 3, 3))


MESHES = {
    1: np.array(FLOOR_TRIANGLE, np.float64),
    2: np.array(FLOOR_QUAD, np.float64),
    # (between the floor and the first light of config 3, facing up)
    3: np.array(FLOOR_QUAD + [[[-2.5, 1.0, 1.0], [-0.5, 1.0, 1.0], [-1.5, 3.0, 1.0]]], np.float64),
    17: np.concatenate([np.array(FLOOR_QUAD, np.float64), small_triangles(15)], 0),
}


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    """one dataset per mesh, written once"""
    out = {}
    for count, positions in MESHES.items():
        dataset = synthetic.write_dataset(str(tmp_path_factory.mktemp("mesh_%d" % count)), grid=8, box_count=0, ltc_resolution=16, fresnel_count=8)
        normals = np.cross(positions[:, 1] - positions[:, 0], positions[:, 2] - positions[:, 0])
        normals /= np.linalg.norm(normals, axis=-1, keepdims=True)
        names = synthetic.write_material_textures(dataset["textures"])
        synthetic.write_vks(dataset["scene"], positions, np.repeat(normals[:, None, :], 3, 1), positions[:, :, :2] * 0.5, np.zeros(len(positions), np.uint8), names)
        out[count] = dataset
    return out


@pytest.fixture(scope="module")
def oracle_bvhs():
    """the oracle's tree per mesh: the same for every builder"""
    return {}


@pytest.mark.parametrize("count", sorted(MESHES))
@pytest.mark.parametrize("builder", BUILDERS)
def test_small_mesh_is_built_and_shaded_like_the_oracle(datasets, oracle_bvhs, builder, count):
    r = renderer.Renderer()
    renderer.setup_config(r, 3, datasets[count], width=WIDTH, height=HEIGHT, acceleration_structure=builder)
    r.create_targets()
    r.create_pass()
    r.render_visibility()
    r.render()
    image, visibility, rays = r.read_radiance(), r.read_visibility(), r.last_ray_count()
    s = r.app.scene.acceleration_structure
    tree = {k: int(getattr(s, k)) for k in ("node_count", "leaf_count", "builder", "wide_node_count", "wide_stack_need")}
    tree["wide_nodes"], tree["build_ms"], triangles = bool(s.wide_nodes), float(s.build_milliseconds), int(r.app.scene.mesh.triangle_count)
    cam = r.app.scene_specification.camera
    cpu, inputs, oracle_bvhs[count] = oracle_render(r, visibility=visibility, math_mode=renderer.ORACLE_MATH_MODE[r.arithmetic], bvh=oracle_bvhs.get(count))
    cpu_visibility = oracle.primary_visibility(inputs["constants"], oracle_bvhs[count], WIDTH, HEIGHT, cam.near, cam.far)
    r.close()
    print(tree, triangles, rays)
    assert triangles == count and tree["leaf_count"] >= count
    assert tree["node_count"] == 2 * tree["leaf_count"] - 1
    assert tree["builder"] == renderer.BVH_BUILDER[builder]
    assert tree["build_ms"] > 0.0
    assert (visibility != 0xFFFFFFFF).mean() > 0.2
    assert np.array_equal(visibility, cpu_visibility), "%d pixels differ" % int((visibility != cpu_visibility).sum())
    assert compare(image, cpu)["bit_exact"], compare(image, cpu)
    assert rays > 0
    if count == 1:
        # a single leaf has nothing to collapse: the rays walk the binary tree, and are still counted
        assert not tree["wide_nodes"] and tree["wide_node_count"] == 0
    else:
        assert tree["wide_nodes"] and tree["wide_node_count"] >= 1
