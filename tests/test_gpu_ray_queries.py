"""The ray queries for the caller's rays (include/vkr_ray_queries.h, csrc/ray_queries.hip) against the numpy brute force
of vulkan_renderer_amd/ray_queries.py, which tests/test_ray_queries.py pins to the oracle: the primitive and the bits of
t, u, v of every ray, for every walk, builder and query, on a tree with split triangles, through the spill buffer of the
wide walk, for the special rays of the contract, at the ends of the host control flow, on a caller's stream, against
the visibility pass, and the refusals."""
import ctypes as C

import numpy as np
import pytest

from helpers import DeviceBuffer
from vulkan_renderer_amd import capi, ray_queries as rq, renderer, synthetic

pytestmark = pytest.mark.gpu

RAY_COUNT = 4097  # no multiple of 64 or 256
BUILDERS = ("sah_device", "lbvh_device", "sah_host")
WALKS = ("binary", "wide", "auto")
# few towers, fences and louvres: about 4 000 triangles, the long thin ones split into several leaves by the device SAH build
SMALL_LARGE_SCENE = dict(grid=24, tower_count=6, sphere_count=0, fence_count=6, louvre_count=3)


def canonical_bits(values):
    """the bits of floats, every NaN the same (the sign and payload of a NaN are not part of the contract)"""
    values = np.ascontiguousarray(values, np.float32)
    return np.where(np.isnan(values), np.uint32(0x7FC00000), values.view(np.uint32))


def assert_same_hits(got, expected, what=""):
    wrong = np.nonzero(got["primitive"] != expected["primitive"])[0]
    assert len(wrong) == 0, (what, len(wrong), wrong[:5], got[wrong[:5]], expected[wrong[:5]])
    for field in ("t", "u", "v"):
        wrong = np.nonzero(canonical_bits(got[field]) != canonical_bits(expected[field]))[0]
        assert len(wrong) == 0, (what, field, len(wrong), wrong[:5], got[wrong[:5]], expected[wrong[:5]])


def special_rays(vertices, regular, regular_hits):
    """The special rays of the contract, each judged by the rule like any other ray"""
    ground = float(vertices[0, 0, 2])
    o, rays = [0.31, 0.17, 1.5], []

    def add(origin, direction, t_min=1.0e-3, t_max=1.0e3):
        rays.append(rq.make_rays([origin], [direction], t_min, t_max))

    # axis-parallel directions, +0 and -0 components
    for direction in ([0.0, 0.0, -1.0], [-0.0, 0.0, -1.0], [0.0, -0.0, -1.0], [-0.0, -0.0, -2.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [-1.0, -0.0, 0.0],
                      [0.0, 1.0, -0.0], [-0.0, -3.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, -1.0], [-1.0, 0.0, -1.0]):
        add(o, direction)
        add([0.31, 0.17, 0.3], direction)
        # (on a grid line of the ground and on a vertex of it)
        add([0.0, 0.0, 1.0], direction)
    # origins on the ground plane: t = 0 is excluded by t_min; in the plane every determinant vanishes or nearly so
    for direction in ([0.3, 0.1, -1.0], [0.3, 0.1, 1.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, -1.0]):
        add([0.31, 0.17, ground], direction)
        add([0.0, 0.0, ground], direction, 0.0)
        add([0.31, 0.17, ground], direction, -1.0)
    # t_max equal to the winner's t, one float below and one above it; t_min likewise
    hit = np.nonzero(regular_hits["primitive"] != rq.NO_PRIMITIVE)[0][:40]
    for i in hit:
        t = regular_hits["t"][i]
        for t_max in (t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(np.inf))):
            add(regular["origin"][i], regular["direction"][i], 1.0e-3, t_max)
        for t_min in (t, np.nextafter(t, np.float32(np.inf))):
            add(regular["origin"][i], regular["direction"][i], t_min, 1.0e3)
    # outside the scene box, pointing away and back, near enough for the boxes and too far for them
    for origin in ([25.0, 25.0, 5.0], [-24.0, 3.0, 0.5], [40.0, 40.0, 5.0], [3.0, 2.0, 700.0], [1.0e6, 2.0e6, 1.0e6], [-3.0e9, 1.0, 2.0]):
        away = np.array(origin) / np.linalg.norm(origin)
        add(origin, away)
        add(origin, -away, 1.0e-3, np.inf)
        add(origin, [0.3 - origin[0], 0.2 - origin[1], 0.0 - origin[2]], 1.0e-3, 2.0)
    # t_max = +infinity, negative t_min
    for i in range(24):
        add(regular["origin"][i], regular["direction"][i], 1.0e-3, np.inf)
        add(regular["origin"][i], regular["direction"][i], -np.inf if i % 2 else -5.0, np.inf)
    # empty intervals, zero directions
    add(o, [0.1, 0.2, -1.0], 2.0, 1.0)
    add(o, [0.1, 0.2, -1.0], np.inf, -np.inf)
    add(o, [0.0, 0.0, 0.0])
    add(o, [0.0, -0.0, 0.0])
    # NaN in every one of the eight floats
    for j in range(8):
        ray = rq.make_rays([o], [[0.1, 0.2, -1.0]], 1.0e-3, 1.0e3)
        ray.view(np.float32)[j] = np.nan
        rays.append(ray)
    # infinite and huge components, tiny directions
    for big in (np.inf, -np.inf, 1.0e30, -3.0e38):
        add([big, 0.2, 1.0], [0.1, 0.2, -1.0])
        add([0.3, 0.2, big], [0.1, 0.2, -1.0])
        add(o, [big, 0.2, -1.0])
        add(o, [0.1, big, -1.0])
        add(o, [big, big, big])
        add(o, [0.0, 0.0, big])
    add(o, [1.0e-30, 2.0e-30, -1.0e-29], 1.0e-3, np.inf)
    add(o, [0.0, 0.0, -1.0e-40], 1.0e-3, np.inf)
    add(o, [0.1, 0.2, -1.0], -np.inf, np.inf)
    return np.concatenate(rays)


class Case:
    """a geometry with its rays and their answers by the brute force (computed once), and the renderers that hold its trees"""

    def __init__(self, dataset):
        self.dataset, self.renderers = dataset, {}
        r = self.renderer("sah_device")
        inputs = r.host_inputs()
        self.vertices = rq.dequantize(inputs["quantized_positions"], inputs["dequantization_factor"], inputs["dequantization_summand"])
        regular = rq.test_rays(self.vertices, RAY_COUNT, 11)
        self.rays = np.concatenate([regular, special_rays(self.vertices, regular, rq.closest_hits_brute_force(self.vertices, regular, False))])
        self.expected = {"two_sided": rq.closest_hits_brute_force(self.vertices, self.rays, False), "culled": rq.closest_hits_brute_force(self.vertices, self.rays, True),
                         "any": rq.any_hits_brute_force(self.vertices, self.rays)}

    def renderer(self, builder):
        if builder not in self.renderers:
            r = renderer.Renderer()
            renderer.setup_config(r, 3, self.dataset, width=64, height=48, acceleration_structure=builder)
            self.renderers[builder] = r
        return self.renderers[builder]

    def query(self, r, query, walk, rays=None, **options):
        rays = self.rays if rays is None else rays
        if query == "any":
            return r.trace_any_hits(rays["origin"], rays["direction"], rays["t_min"], rays["t_max"], walk=walk, **options)
        return r.trace_closest_hits(rays["origin"], rays["direction"], rays["t_min"], rays["t_max"], cull_back_faces=query == "culled", walk=walk, **options)

    def check(self, r, query, walk, count=None, **options):
        rays = self.rays if count is None else self.rays[:count]
        got, expected = self.query(r, query, walk, rays, **options), self.expected[query][:len(rays)]
        assert len(got) == len(rays)
        if query == "any":
            wrong = np.nonzero(got != expected)[0]
            assert len(wrong) == 0, (query, walk, len(wrong), wrong[:5], rays[wrong[:5]])
        else:
            assert_same_hits(got, expected, (query, walk))

    def close(self):
        for r in self.renderers.values():
            r.close()


@pytest.fixture(scope="module")
def cases(dataset, tmp_path_factory):
    out = {"dataset": Case(dataset),
           "split": Case(synthetic.write_dataset(str(tmp_path_factory.mktemp("small_large_scene")), seed=4321, ltc_resolution=16, fresnel_count=8, large=SMALL_LARGE_SCENE))}
    yield out
    for case in out.values():
        case.close()


TREES = [("dataset", builder) for builder in BUILDERS] + [("split", "sah_device")]


def test_the_rays_are_worth_tracing(cases):
    for name, case in cases.items():
        two_sided, culled, blocked = case.expected["two_sided"], case.expected["culled"], case.expected["any"]
        regular = slice(0, RAY_COUNT)
        print(name, len(case.vertices), "triangles,", len(case.rays), "rays,", int(blocked.sum()), "blocked,", int((culled["primitive"] != two_sided["primitive"]).sum()), "decided by culling")
        assert 0.5 < blocked[regular].mean() < 1.0
        assert (culled["primitive"][regular] != two_sided["primitive"][regular]).sum() > 50
        assert len(case.rays) % 64 != 0 and len(case.rays) > RAY_COUNT + 300
    structure = cases["split"].renderer("sah_device").app.scene.acceleration_structure
    triangles = int(cases["split"].renderer("sah_device").app.scene.mesh.triangle_count)
    print("split scene:", triangles, "triangles in", int(structure.leaf_count), "leaves")
    # split triangles are really walked: a hit must be reported once, whichever of its leaves are visited
    assert structure.leaf_count > triangles
    assert int(cases["dataset"].renderer("sah_device").app.scene.mesh.triangle_count) == 8480


@pytest.mark.parametrize("query", ["two_sided", "culled", "any"])
@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("scene, builder", TREES)
def test_answers_equal_the_brute_force(cases, scene, builder, walk, query):
    case = cases[scene]
    r = case.renderer(builder)
    structure = r.app.scene.acceleration_structure
    assert structure.builder == renderer.BVH_BUILDER[builder] and structure.wide_nodes
    case.check(r, query, walk)


@pytest.mark.parametrize("query", ["any", "two_sided", "culled"])
@pytest.mark.parametrize("scene, builder", [("dataset", "sah_device"), ("dataset", "lbvh_device"), ("split", "sah_device")])
def test_stack_entries_beyond_lds_spill_to_device_memory(cases, scene, builder, query):
    """With four entries in LDS the deeper ones go through the buffer in device memory.  Some ray must get there:
    the rays that are tested against every triangle (infinite components among the specials) push every child of every
    node, so their stacks reach the worst case of the build, wide_stack_need."""
    case = cases[scene]
    r = case.renderer(builder)
    need = int(r.app.scene.acceleration_structure.wide_stack_need)
    print(scene, builder, "wide_stack_need", need)
    assert need > 4 and np.isinf(case.rays["direction"]).any() and np.isinf(case.rays["origin"]).any()
    case.check(r, query, "wide", lds_stack_entries=4)
    case.check(r, query, "wide", lds_stack_entries=1)


# ---- the ends of the host control flow ----------------------------------------------------------------------------------

@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 257])
def test_ray_counts_around_the_wave_and_the_workgroup(cases, count):
    case = cases["dataset"]
    r = case.renderer("sah_device")
    for walk in WALKS:
        for query in ("two_sided", "culled", "any"):
            case.check(r, query, walk, count=count)
    case.check(r, "two_sided", "wide", count=count, lds_stack_entries=2)
    case.check(r, "any", "wide", count=count, lds_stack_entries=2)


def small_meshes():
    from test_gpu_bvh_small_meshes import MESHES
    return MESHES


@pytest.mark.parametrize("count", [1, 2, 3, 17])
@pytest.mark.parametrize("builder", BUILDERS)
def test_meshes_of_a_few_triangles(tmp_path, builder, count):
    """trees that are a single leaf (no wide tree: the wide walk is refused, auto walks the binary tree), two leaves, three, seventeen"""
    positions = small_meshes()[count]
    dataset = synthetic.write_dataset(str(tmp_path / "mesh"), grid=8, box_count=0, ltc_resolution=16, fresnel_count=8)
    normals = np.cross(positions[:, 1] - positions[:, 0], positions[:, 2] - positions[:, 0])
    normals /= np.linalg.norm(normals, axis=-1, keepdims=True)
    names = synthetic.write_material_textures(dataset["textures"])
    stored = synthetic.write_vks(dataset["scene"], positions, np.repeat(normals[:, None, :], 3, 1), positions[:, :, :2] * 0.5, np.zeros(len(positions), np.uint8), names)
    vertices = rq.dequantize(stored["quantized_positions"], stored["dequantization_factor"], stored["dequantization_summand"])
    regular = rq.test_rays(vertices, 321, 5)
    rays = np.concatenate([regular, special_rays(vertices, regular, rq.closest_hits_brute_force(vertices, regular, False))])
    r = renderer.Renderer()
    try:
        renderer.setup_config(r, 3, dataset, width=64, height=48, acceleration_structure=builder)
        structure = r.app.scene.acceleration_structure
        assert int(r.app.scene.mesh.triangle_count) == count and bool(structure.wide_nodes) == (count > 1)
        for walk in WALKS:
            if count == 1 and walk.startswith("wide"):
                with pytest.raises(RuntimeError):
                    r.trace_any_hits(rays["origin"], rays["direction"], rays["t_min"], rays["t_max"], walk=walk)
                continue
            for cull in (False, True):
                got = r.trace_closest_hits(rays["origin"], rays["direction"], rays["t_min"], rays["t_max"], cull_back_faces=cull, walk=walk, lds_stack_entries=2 if cull else 0)
                assert_same_hits(got, rq.closest_hits_brute_force(vertices, rays, cull), (walk, cull))
            assert np.array_equal(r.trace_any_hits(rays["origin"], rays["direction"], rays["t_min"], rays["t_max"], walk=walk), rq.any_hits_brute_force(vertices, rays))
    finally:
        r.close()


def test_device_pointers_on_a_stream_of_the_caller(cases):
    """nothing is copied and nothing waits: the call orders its kernels on the caller's stream, and a second call on the
    same stream may read what the first one wrote"""
    case = cases["split"]
    r = case.renderer("sah_device")
    hip = C.CDLL("libamdhip64.so")
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    rays, hits, blocked = DeviceBuffer(case.rays.nbytes), DeviceBuffer(16 * len(case.rays)), DeviceBuffer(len(case.rays))
    try:
        rays.upload(case.rays)
        for walk, query, lds in (("binary", "culled", 0), ("wide", "two_sided", 0), ("wide", "culled", 3), ("auto", "two_sided", 0)):
            assert r.trace_closest_hits(rays_pointer=rays.ptr, hits_pointer=hits.ptr, count=len(case.rays), cull_back_faces=query == "culled", walk=walk, lds_stack_entries=lds, stream=stream) is None
            assert r.trace_any_hits(rays_pointer=rays.ptr, blocked_pointer=blocked.ptr, count=len(case.rays), walk=walk, lds_stack_entries=lds, stream=stream) is None
            assert hip.hipStreamSynchronize(stream) == 0
            assert_same_hits(hits.download(len(case.rays), rq.HIT), case.expected[query], (walk, query))
            assert np.array_equal(blocked.download(len(case.rays), np.uint8), case.expected["any"].astype(np.uint8))
            hits.zero()
            blocked.zero()
        # host arrays on the caller's stream: uploaded, traced there, waited for and read back; and the calls of two
        # streams share the device's stack buffer, one after the other
        some = case.rays[:RAY_COUNT]
        for handle in (stream, stream.value):
            got = r.trace_closest_hits(some["origin"], some["direction"], some["t_min"], some["t_max"], walk="wide", lds_stack_entries=3, stream=handle)
            assert_same_hits(got, case.expected["two_sided"][:RAY_COUNT], "host arrays on a stream")
            got = r.trace_any_hits(some["origin"], some["direction"], some["t_min"], some["t_max"], walk="wide", lds_stack_entries=3)
            assert np.array_equal(got, case.expected["any"][:RAY_COUNT])
        assert r.trace_any_hits(rays_pointer=rays.ptr, blocked_pointer=blocked.ptr, count=len(case.rays), walk="wide", lds_stack_entries=3, stream=stream) is None
        assert np.array_equal(r.trace_any_hits(rays_pointer=rays.ptr, count=len(case.rays), walk="wide", lds_stack_entries=3), case.expected["any"])
        assert hip.hipStreamSynchronize(stream) == 0
        assert np.array_equal(blocked.download(len(case.rays), np.uint8), case.expected["any"].astype(np.uint8))
    finally:
        for buffer in (rays, hits, blocked):
            buffer.free()
        hip.hipStreamDestroy(stream)


# ---- the existing door, cross-checked ---------------------------------------------------------------------------------

@pytest.mark.parametrize("config", [1, 3])
def test_pixel_rays_see_what_the_visibility_pass_sees(dataset, config):
    r = renderer.Renderer()
    try:
        renderer.setup_config(r, config, dataset, width=64, height=48, acceleration_structure="sah_device")
        r.create_targets()
        r.create_pass()
        r.render_visibility()
        visibility = r.read_visibility()
        rays = r.pixel_rays()
        assert len(rays) == 64 * 48 and (visibility != 0xFFFFFFFF).mean() > 0.2
        for walk in WALKS:
            hits = r.trace_closest_hits(rays["origin"], rays["direction"], rays["t_min"], rays["t_max"], cull_back_faces=True, walk=walk)
            assert np.array_equal(hits["primitive"].reshape(48, 64), visibility), walk
        for x, y in ((0, 0), (63, 47), (31, 24), (5, 40), (60, 3)):
            picked = r.pick(x, y)
            assert picked["primitive"] == visibility[y, x]
            assert (picked["primitive"] == 0xFFFFFFFF) == np.isinf(picked["t"])
        with pytest.raises(ValueError):
            r.pick(64, 0)
    finally:
        r.close()


def test_the_depth_command_writes_the_depth_of_the_camera_rays(dataset, tmp_path):
    out = tmp_path / "depth.npy"
    assert rq.main([dataset["scene"], "--depth", str(out), "--width", "40", "--height", "24"]) == 0
    depth = np.load(out)
    assert depth.shape == (24, 40) and depth.dtype == np.float32
    assert np.isfinite(depth).mean() > 0.2 and (depth[np.isfinite(depth)] >= 0.05).all()


# ---- refusals -----------------------------------------------------------------------------------------------------------

def refusals():
    def no_structure(scene, device, options):
        return capi.Scene(), device, 64, options

    def no_device(scene, device, options):
        return scene, None, 64, options

    def too_many(scene, device, options):
        return scene, device, (1 << 31) + 1, options

    def no_wide_tree(scene, device, options):
        scene.acceleration_structure.wide_nodes = None
        return scene, device, 64, capi.RayQueryOptions(rq.WALK["wide"], 0)

    def deep_wide_tree(scene, device, options):
        scene.acceleration_structure.wide_stack_need = rq.WIDE_STACK_MAX + 1
        return scene, device, 64, capi.RayQueryOptions(rq.WALK["wide"], 0)

    def too_much_lds(scene, device, options):
        return scene, device, 64, capi.RayQueryOptions(rq.WALK["auto"], rq.WIDE_STACK_LDS + 1)

    def no_walk(scene, device, options):
        return scene, device, 64, capi.RayQueryOptions(len(rq.WALK), 0)

    return [no_structure, no_device, too_many, no_wide_tree, deep_wide_tree, too_much_lds, no_walk]


@pytest.mark.parametrize("closest", [True, False], ids=["closest", "any"])
@pytest.mark.parametrize("refusal", refusals(), ids=lambda f: f.__name__)
def test_refusals(cases, capfd, refusal, closest):
    case = cases["dataset"]
    r = case.renderer("sah_device")
    scene, device, count, options = refusal(capi.Scene.from_buffer_copy(r.app.scene), C.byref(r.app.device), None)
    rays, out = DeviceBuffer(32 * 64), DeviceBuffer(16 * 64)
    try:
        rays.upload(case.rays[:64])
        sentinel = np.full(16 * 64, 0xA5, np.uint8)
        out.upload(sentinel)
        # (the library prints through C's buffered stdout: what earlier calls left there goes first)
        C.CDLL(None).fflush(None)
        capfd.readouterr()
        options = C.byref(options) if options is not None else None
        if closest:
            assert r.lib.trace_closest_hits(C.byref(scene), device, rays.ptr, count, 0, out.ptr, options, None) == 1
        else:
            assert r.lib.trace_any_hits(C.byref(scene), device, rays.ptr, count, out.ptr, options, None) == 1
        C.CDLL(None).fflush(None)
        assert len(capfd.readouterr().out.strip().splitlines()) == 1
        assert np.array_equal(out.download(16 * 64, np.uint8), sentinel)
        # ... and the same buffers are filled when nothing is wrong
        assert r.lib.trace_any_hits(C.byref(r.app.scene), C.byref(r.app.device), rays.ptr, 64, out.ptr, None, None) == 0
        assert np.array_equal(out.download(64, np.uint8), case.expected["any"][:64].astype(np.uint8))
    finally:
        rays.free()
        out.free()
