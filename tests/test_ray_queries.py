"""The numpy restatement of the ray queries (vulkan_renderer_amd/ray_queries.py; the rules: include/vkr_ray_queries.h)
against something that does not come from it - the oracle's closest front hit and any hit (oracle/oracle_bvh.c), whose
triangle test the device's is pinned to.  The GPU tests compare the kernels with the restatement bit for bit."""
import ctypes as C

import numpy as np
import pytest

import oracle
from vulkan_renderer_amd import ray_queries as rq, synthetic

# (grid, boxes, rays): with seed 7, 4 466 / 1 281 / 3 934 of these rays have a runner-up at exactly the winner's t
SCENES = [(16, 8, 9000), (32, 24, 3000), (64, 24, 9000)]


class OracleBvh(C.Structure):
    """how bvh_t of oracle/oracle_bvh.c begins (the struct is private: test_dequantize_... checks what it can of this)"""
    _fields_ = [("vertices", C.POINTER(C.c_float)), ("triangle_count", C.c_uint64), ("order", C.POINTER(C.c_uint32)), ("nodes", C.c_void_p), ("node_count", C.c_uint32)]


def oracle_library():
    lib = oracle.lib()
    fp = C.POINTER(C.c_float)
    lib.oracle_bvh_closest_front_hit.restype = C.c_uint32
    lib.oracle_bvh_closest_front_hit.argtypes = [C.c_void_p, fp, fp, C.c_float, C.c_float]
    lib.oracle_bvh_any_hit.restype = C.c_int
    return lib


def make_case(directory, grid, box_count, ray_count):
    positions, normals, uvs, materials = synthetic.make_scene_geometry(grid, box_count, seed=1234)
    stored = synthetic.write_vks(str(directory / "scene.vks"), positions, normals, uvs, materials, ["a", "b", "c"])
    vertices = rq.dequantize(stored["quantized_positions"], stored["dequantization_factor"], stored["dequantization_summand"])
    bvh = oracle.Bvh(stored["quantized_positions"], stored["dequantization_factor"], stored["dequantization_summand"])
    return {"stored": stored, "vertices": vertices, "bvh": bvh, "rays": rq.test_rays(vertices, ray_count, 7)}


@pytest.fixture(scope="module", params=SCENES, ids=lambda s: "grid%d_boxes%d" % s[:2])
def case(request, tmp_path_factory):
    """a scene as it is stored in a file, its vertices by the restatement, the oracle's tree and the rays, made once"""
    return make_case(tmp_path_factory.mktemp("scene"), *request.param)


def test_dequantize_equals_the_vertices_of_the_oracle_tree(case):
    """dequantize() is the rule of oracle_bvh.c:84-92 - multiply, then add: two roundings - so it gives the vertices that
    the oracle's tree holds (the first member of its bvh_t), every bit of every vertex.  oracle_decode_position is the
    decode of the shading path, which fuses the two operations (mesh_quantization.glsl:38-45): it may differ from the
    geometry of the ray queries in the last bit, and does for some vertices."""
    stored, vertices = case["stored"], case["vertices"]
    # The handle of oracle.Bvh points to the private bvh_t of oracle_bvh.c:28-35, which is assumed to begin like OracleBvh
    # below.  What can be checked of that is: the triangle count sits behind the vertices, the order behind
    # it holds every triangle once, and the node count is that of a binary tree.  (If the struct is ever reordered, this fails here and not
    # in the comparison of the bits, or reads as garbage that the 1-ulp comparison with oracle_decode_position catches.)
    tree = C.cast(case["bvh"].handle, C.POINTER(OracleBvh))[0]
    assert tree.triangle_count == len(vertices) and 0 < tree.node_count < 2 * len(vertices)
    assert np.array_equal(np.sort(np.ctypeslib.as_array(tree.order, (len(vertices),))), np.arange(len(vertices)))
    expected = np.ctypeslib.as_array(tree.vertices, (vertices.size,)).reshape(vertices.shape)
    assert vertices.dtype == np.float32 and len(vertices) == len(stored["material_indices"])
    assert np.array_equal(vertices.view(np.uint32), expected.view(np.uint32))
    lib, fp = oracle.lib(), C.POINTER(C.c_float)
    factor, summand = (np.ascontiguousarray(stored[k], np.float32) for k in ("dequantization_factor", "dequantization_summand"))
    out, flat = np.zeros(3, np.float32), vertices.reshape(-1, 3)
    for i in np.concatenate([[0, len(flat) - 1], np.random.default_rng(3).integers(0, len(flat), 500)]):
        q0, q1 = (int(w) for w in stored["quantized_positions"][i])
        lib.oracle_decode_position(q0, q1, factor.ctypes.data_as(fp), summand.ctypes.data_as(fp), out.ctypes.data_as(fp))
        assert np.abs(out.view(np.int32).astype(np.int64) - flat[i].view(np.int32)).max() <= 1, i


def test_culled_closest_hit_equals_the_oracle_closest_front_hit(case):
    lib, fp = oracle_library(), C.POINTER(C.c_float)
    rays, handle = case["rays"], case["bvh"].handle
    hits, runner_up = rq.closest_and_runner_up(case["vertices"], rays, True)
    assert np.array_equal(hits.view(np.uint32), rq.closest_hits_brute_force(case["vertices"], rays, True).view(np.uint32))
    expected = np.array([lib.oracle_bvh_closest_front_hit(handle, r["origin"].ctypes.data_as(fp), r["direction"].ctypes.data_as(fp), r["t_min"], r["t_max"]) for r in rays], np.uint32)
    differing = np.nonzero(hits["primitive"] != expected)[0]
    ties = int((runner_up == hits["t"]).sum())
    print("%d rays, %d hit, %d exact ties in t, %d differ from the oracle" % (len(rays), int((hits["primitive"] != rq.NO_PRIMITIVE).sum()), ties, len(differing)))
    # The oracle's loop tests against the shrunk t_max, so its answer depends on its visiting order in principle: a ray
    # that differs must be a near tie (runner-up within 8 ulps of the winner), and there may be at most 0.1 % of them
    for i in differing:
        gap = abs(int(runner_up[i].view(np.uint32)) - int(hits["t"][i].view(np.uint32)))
        assert gap <= 8, (i, rays[i], hits[i], expected[i], gap)
    assert len(differing) <= len(rays) // 1000
    assert (hits["primitive"] != rq.NO_PRIMITIVE).mean() > 0.5 and ties > 100


def test_any_hit_equals_the_oracle_with_and_without_its_tree(case):
    lib, fp = oracle_library(), C.POINTER(C.c_float)
    rays, handle = case["rays"], case["bvh"].handle
    blocked = rq.any_hits_brute_force(case["vertices"], rays)
    for brute_force in (1, 0):
        expected = np.array([lib.oracle_bvh_any_hit(handle, r["origin"].ctypes.data_as(fp), r["direction"].ctypes.data_as(fp), r["t_min"], r["t_max"], brute_force) for r in rays], bool)
        assert np.array_equal(blocked, expected), (brute_force, int((blocked != expected).sum()))
    # two-sided closest hits and any hits are the same question
    two_sided = rq.closest_hits_brute_force(case["vertices"], rays, False)
    assert np.array_equal(two_sided["primitive"] != rq.NO_PRIMITIVE, blocked)
    assert 0.3 < blocked.mean() < 1.0


def test_values_of_a_hit_lie_on_the_triangle(case):
    """t, u, v are what they claim to be: o + t d is the barycentric combination, to rounding"""
    rays, vertices = case["rays"][:600], case["vertices"].astype(np.float64)
    hits = rq.closest_hits_brute_force(case["vertices"], rays, False)
    hit = hits["primitive"] != rq.NO_PRIMITIVE
    v = vertices[hits["primitive"][hit]]
    u_, v_ = hits["u"][hit].astype(np.float64)[:, None], hits["v"][hit].astype(np.float64)[:, None]
    on_triangle = (1 - u_ - v_) * v[:, 0] + u_ * v[:, 1] + v_ * v[:, 2]
    on_ray = rays["origin"][hit].astype(np.float64) + hits["t"][hit].astype(np.float64)[:, None] * rays["direction"][hit]
    assert hit.sum() > 300 and np.abs(on_triangle - on_ray).max() < 1.0e-3
    assert ((hits["t"][hit] >= rays["t_min"][hit]) & (hits["t"][hit] <= rays["t_max"][hit])).all()


def test_degenerate_rays_miss(case):
    """rule 6, and what the triangle test makes of such rays on its own"""
    vertices = case["vertices"]
    down = rq.make_rays([[0.3, 0.2, 1.0]] * 8, [[0.1, 0.05, -1.0]] * 8, 1.0e-3, 1.0e3)
    assert rq.closest_hits_brute_force(vertices, down[:1], False)["primitive"][0] != rq.NO_PRIMITIVE
    down["t_min"][1], down["t_max"][1] = 2.0, 1.0
    down["direction"][2] = 0.0
    down["direction"][3] = [0.0, -0.0, 0.0]
    down["origin"][4, 1] = np.nan
    down["direction"][5, 0] = np.nan
    down["t_min"][6] = np.nan
    down["t_max"][7] = np.nan
    assert rq.degenerate(down).tolist() == [False] + [True] * 7
    for cull in (False, True):
        hits = rq.closest_hits_brute_force(vertices, down, cull)
        assert hits["primitive"][0] != rq.NO_PRIMITIVE
        assert np.array_equal(hits[1:].view(np.uint32), np.repeat(rq.misses(), 7).view(np.uint32))
    assert rq.any_hits_brute_force(vertices, down).tolist() == [True] + [False] * 7
    miss = rq.misses()[0]
    assert miss["primitive"] == 0xFFFFFFFF and miss["t"] == np.inf and miss["u"] == 0 and miss["v"] == 0
    assert rq.RAY.itemsize == 32 and rq.HIT.itemsize == 16


def test_pixel_rays_restate_the_visibility_kernel(tmp_path):
    """the rays of pixel_rays() give the oracle's primary visibility: same bytes, same operation order"""
    from vulkan_renderer_amd import renderer
    case = make_case(tmp_path, 16, 8, 0)
    scene = renderer.HostScene()
    camera = synthetic.DEFAULT_CAMERA
    scene.set_camera(camera["position"], camera["rotation_x"], camera["rotation_z"], camera["vertical_fov"], camera["near"], camera["far"])
    scene.app.swapchain.extent.width, scene.app.swapchain.extent.height = 48, 27
    constants = scene.constants()
    scene.close()
    rays = rq.pixel_rays(constants, 48, 27, camera["near"], camera["far"])
    expected = oracle.primary_visibility(constants, case["bvh"], 48, 27, camera["near"], camera["far"])
    hits = rq.closest_hits_brute_force(case["vertices"], rays, True)
    assert (expected != 0xFFFFFFFF).mean() > 0.2
    assert np.array_equal(hits["primitive"].reshape(27, 48), expected)
