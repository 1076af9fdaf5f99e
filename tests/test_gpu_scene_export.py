"""Scenes exported on the GPU (include/vkr_scene_export.h export_scene, csrc/scene_export.hip) against their numpy
restatement (vulkan_renderer_amd/scene_export.py, pinned by tests/test_scene_export.py) and against the files of the
reference's add-on in every byte, the error returns, and a frame shaded from an exported file against the CPU oracle in
every bit."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import golden_cases
import scene_export_cases as cases
from helpers import oracle_render
from vulkan_renderer_amd import capi, renderer, synthetic
from vulkan_renderer_amd import scene_export as se

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def device():
    r = renderer.Renderer()
    yield r
    r.close()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "scene_export.npz"))


@functools.lru_cache(maxsize=None)
def large_mesh():
    """300 000 triangles over 200 000 vertices: the sort runs more than one tile per pass, and several hundred Morton codes
    are equal - the only thing that tests that such triangles keep their order"""
    return cases.random_mesh(200000, 300000, seed=7)


# 1: one lane; 61: less than a wave; 3 000: several workgroups, the last one partial
@pytest.mark.parametrize("sort_triangles", [False, True], ids=["unsorted", "sorted"])
@pytest.mark.parametrize("vertex_count,triangle_count", [(3, 1), (40, 61), (1500, 3000)])
def test_device_equals_the_restatement(device, vertex_count, triangle_count, sort_triangles):
    mesh = cases.random_mesh(vertex_count, triangle_count, seed=11)
    differing = cases.buffers_differ(device.export_scene(sort_triangles=sort_triangles, **mesh), se.export(sort_triangles=sort_triangles, **mesh))
    assert not differing, "bytes that differ per buffer: %r" % (differing,)


@pytest.mark.parametrize("sort_triangles", [False, True], ids=["unsorted", "sorted"])
def test_device_writes_the_files_of_the_addon(device, golden, tmp_path, sort_triangles):
    for name in ("small", "medium"):
        path = str(tmp_path / (name + ".vks"))
        device.export_scene(sort_triangles=sort_triangles, path=path, **cases.golden_mesh(golden, name))
        got, expected = open(path, "rb").read(), golden["%s_file_%s" % (name, "sorted" if sort_triangles else "unsorted")].tobytes()
        assert len(got) == len(expected)
        differing = int((np.frombuffer(got, np.uint8) != np.frombuffer(expected, np.uint8)).sum())
        assert differing == 0, "%s: %d bytes differ" % (name, differing)


@pytest.mark.parametrize("sort_triangles", [False, True], ids=["unsorted", "sorted"])
def test_large_mesh_equals_the_restatement(device, sort_triangles):
    mesh = large_mesh()
    if sort_triangles:
        tied = 300000 - np.unique(se.morton_codes(mesh["positions"], mesh["indices"])).size
        assert tied > 300, "the mesh is meant to have several hundred triangles of equal code, it has %d" % tied
    differing = cases.buffers_differ(device.export_scene(sort_triangles=sort_triangles, **mesh), se.export(sort_triangles=sort_triangles, **mesh))
    assert not differing, "bytes that differ per buffer: %r" % (differing,)


@pytest.mark.parametrize("sort_triangles", [False, True], ids=["unsorted", "sorted"])
@pytest.mark.parametrize("name", sorted(cases.EDGE_MESHES))
def test_edge_inputs_equal_the_restatement(device, name, sort_triangles):
    mesh = cases.EDGE_MESHES[name]()
    differing = cases.buffers_differ(device.export_scene(sort_triangles=sort_triangles, **mesh), se.export(sort_triangles=sort_triangles, **mesh))
    assert not differing, "bytes that differ per buffer: %r" % (differing,)


def refused_changes():
    mesh = cases.random_mesh(40, 61, seed=11)
    changes = {}
    changes["index_out_of_range"] = dict(indices=mesh["indices"].copy())
    changes["index_out_of_range"]["indices"][60, 2] = 40
    changes["huge_index"] = dict(indices=mesh["indices"].copy())
    changes["huge_index"]["indices"][0, 0] = 0xFFFFFFFF
    changes["material_index_out_of_range"] = dict(material_indices=mesh["material_indices"].copy())
    changes["material_index_out_of_range"]["material_indices"][7] = 3
    changes["nan_position"] = dict(positions=mesh["positions"].copy())
    changes["nan_position"]["positions"][39, 1] = np.nan
    changes["infinite_normal"] = dict(normals=mesh["normals"].copy())
    changes["infinite_normal"]["normals"][0, 2] = -np.inf
    changes["infinite_tex_coord"] = dict(tex_coords=mesh["tex_coords"].copy())
    changes["infinite_tex_coord"]["tex_coords"][60, 2, 1] = np.inf
    changes["no_triangles"] = dict(indices=np.zeros((0, 3), np.uint32), tex_coords=None, material_indices=None)
    changes["no_materials"] = dict(material_names=())
    changes["too_many_materials"] = dict(material_names=("m",) * 257)
    return mesh, changes


@pytest.mark.parametrize("sort_triangles", [False, True], ids=["unsorted", "sorted"])
@pytest.mark.parametrize("name", sorted(refused_changes()[1]))
def test_invalid_input_is_refused_and_the_device_goes_on(device, name, sort_triangles):
    """Each returns 1 with the struct zeroed - an index is compared with the vertex count before anything is read through
    it - and a good export on the same device still gives the right bytes"""
    mesh, changes = refused_changes()
    source, keepalive = se.export_source(**{k: v for k, v in dict(mesh, **changes[name]).items()})
    scene = capi.ExportedScene()
    assert device.lib.export_scene(C.byref(scene), device._dev(), C.byref(source), int(sort_triangles)) == 1
    assert bytes(scene) == bytes(C.sizeof(scene))
    with pytest.raises(RuntimeError):
        device.export_scene(sort_triangles=sort_triangles, **dict(mesh, **changes[name]))
    assert not cases.buffers_differ(device.export_scene(sort_triangles=sort_triangles, **mesh), se.export(sort_triangles=sort_triangles, **mesh))


def test_a_triangle_list_with_too_few_vertices_is_refused(device):
    """Without indices triangle t uses the vertices 3 t ... 3 t + 2: they are compared with the vertex count as well"""
    mesh = cases.random_mesh(40, 61, seed=11)
    source, keepalive = se.export_source(mesh["positions"][:39], mesh["normals"][:39])
    source.triangle_count = 14
    scene = capi.ExportedScene()
    for sort_triangles in (0, 1):
        assert device.lib.export_scene(C.byref(scene), device._dev(), C.byref(source), sort_triangles) == 1
        assert bytes(scene) == bytes(C.sizeof(scene))
    source.triangle_count = 13
    assert device.lib.export_scene(C.byref(scene), device._dev(), C.byref(source), 1) == 0
    assert not cases.buffers_differ(se.exported_buffers(scene), se.export(mesh["positions"][:39], mesh["normals"][:39]))
    device.lib.free_exported_scene(C.byref(scene))


def test_export_scene_needs_a_device_and_leaves_it_usable(device):
    mesh = cases.random_mesh(40, 61, seed=11)
    source, keepalive = se.export_source(**mesh)
    scene = capi.ExportedScene()
    assert device.lib.export_scene(C.byref(scene), None, C.byref(source), 1) == 1
    assert bytes(scene) == bytes(C.sizeof(scene))
    assert not cases.buffers_differ(device.export_scene(**mesh), se.export(**mesh))
    assert device.lib.get_scene_export_kernel_milliseconds() > 0.0


def test_obj_file_through_the_command_line_module(device, tmp_path):
    """read_obj() and export_scene() as main() of the module chains them (in this process: main() makes a renderer of its own)"""
    lines = ["usemtl stone.002"]
    mesh = cases.random_mesh(40, 61, seed=11)
    lines += ["v %r %r %r" % tuple(float(x) for x in p) for p in mesh["positions"]]
    lines += ["vn %r %r %r" % tuple(float(x) for x in n) for n in mesh["normals"]]
    lines += ["f " + " ".join("%d//%d" % (i + 1, i + 1) for i in t) for t in mesh["indices"]]
    (tmp_path / "mesh.obj").write_text("\n".join(lines) + "\n")
    assert se.main([str(tmp_path / "mesh.obj"), str(tmp_path / "mesh.vks"), "--no-sort"]) == 0
    expected = se.export(sort_triangles=False, **se.read_obj(str(tmp_path / "mesh.obj")))
    assert expected["material_names"] == ["stone"]
    assert open(tmp_path / "mesh.vks", "rb").read() == se.vks_bytes(expected)
    # (the same corners as the indexed mesh, with the box of the used vertices)
    indexed = se.export(sort_triangles=False, **dict(cases.without_unused_vertices(mesh), tex_coords=None, material_indices=None, material_names=("stone",)))
    assert not cases.buffers_differ(expected, indexed)


def test_a_frame_of_an_exported_scene_equals_the_oracle_bit_for_bit(device, tmp_path):
    """A small synthetic mesh exported on the device, written, read by the unchanged loader with the acceleration
    structure and shaded by the unchanged pass in libm mode; the oracle shades from the same file"""
    dataset = synthetic.write_dataset(str(tmp_path), **dict(golden_cases.DATASET, grid=16, box_count=6))
    names = list(synthetic.DEFAULT_MATERIALS)
    positions, normals, uvs, materials = synthetic.make_scene_geometry(16, 6, golden_cases.DATASET["seed"], materials=len(names))
    exported = device.export_scene(positions, normals, None, uvs, materials, names, path=dataset["scene"])
    restated = se.export(positions, normals, None, uvs, materials, names)
    assert not cases.buffers_differ(exported, restated)
    assert open(dataset["scene"], "rb").read() == se.vks_bytes(restated)
    case = golden_cases.FRAME_CASES[3]
    r = renderer.Renderer(arithmetic="libm")
    golden_cases.apply_case(r, case, dataset)
    assert r.app.scene.mesh.triangle_count == positions.shape[0]
    r.create_targets()
    r.create_pass()
    r.render_visibility()
    r.render()
    image = r.read_radiance()
    visibility = r.read_visibility()
    cpu, inputs, _ = oracle_render(r, visibility=visibility, math_mode=renderer.ORACLE_MATH_MODE["libm"])
    r.close()
    assert np.array_equal(inputs["quantized_positions"], exported["quantized_positions"])
    assert (visibility != 0xFFFFFFFF).mean() > 0.2
    assert not np.isnan(image).any() and image[..., :3].max() > 0.0
    assert np.array_equal(image[..., :3].view(np.uint32), cpu[..., :3].astype(np.float32).view(np.uint32))
