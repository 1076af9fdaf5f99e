"""The scene exporter (include/vkr_scene_export.h) without a GPU: the numpy restatement (vulkan_renderer_amd/scene_export.py),
which the device matches byte for byte (tests/test_gpu_scene_export.py), against the files the reference's Blender add-on
wrote (golden/scene_export.npz, made by golden/make_scene_export.py), the project's own rules where the add-on leaves the
result open, the OBJ reader, the container writer and the unchanged loader."""
import ctypes as C
import os

import numpy as np
import pytest

import scene_export_cases as cases
from vulkan_renderer_amd import capi, renderer
from vulkan_renderer_amd import scene_export as se

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "scene_export.npz"))


@pytest.mark.parametrize("sort_triangles", [False, True], ids=["unsorted", "sorted"])
@pytest.mark.parametrize("name", ["small", "medium"])
def test_restatement_equals_the_files_of_the_addon(golden, name, sort_triangles):
    mesh = cases.golden_mesh(golden, name)
    if sort_triangles:
        # (what makes the add-on's file unique: its argsort is not stable)
        assert np.unique(se.morton_codes(mesh["positions"], mesh["indices"])).size == mesh["indices"].shape[0]
    expected = golden["%s_file_%s" % (name, "sorted" if sort_triangles else "unsorted")].tobytes()
    got = se.vks_bytes(se.export(sort_triangles=sort_triangles, **mesh))
    assert len(got) == len(expected)
    differing = int((np.frombuffer(got, np.uint8) != np.frombuffer(expected, np.uint8)).sum())
    assert differing == 0, "%d bytes differ" % differing


def test_sorting_follows_the_morton_code_with_x_lowest(golden):
    mesh = cases.golden_mesh(golden, "medium")
    codes = se.morton_codes(mesh["positions"], mesh["indices"])
    order = np.argsort(codes, kind="stable")
    plain, ordered = se.export(sort_triangles=False, **mesh), se.export(sort_triangles=True, **mesh)
    T = order.size
    assert np.array_equal(ordered["quantized_positions"].reshape(T, 6), plain["quantized_positions"].reshape(T, 6)[order])
    assert np.array_equal(ordered["normals_and_tex_coords"].reshape(T, 12), plain["normals_and_tex_coords"].reshape(T, 12)[order])
    assert np.array_equal(ordered["material_indices"], plain["material_indices"][order])
    # a step along x alone changes bit 0 of the code: two triangles whose centroids differ in the x cell only
    positions = np.array([(0, 0, 0), (1024, 1024, 1024), (1, 0, 0), (0, 1, 0), (0, 0, 1)], np.float32)
    indices = np.array([(0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3), (4, 4, 4)], np.uint32)
    assert se.morton_codes(positions, indices).tolist() == [0, 0x3FFFFFFF, 1, 2, 4]


@pytest.mark.parametrize("z", [0.0, -0.0])
def test_planar_mesh(z):
    scene = se.export(**cases.planar_mesh(z))
    assert scene["dequantization_factor"][2] == 0.0 and scene["dequantization_factor"][:2].min() > 0.0
    # +0, whatever the sign of the input's zero
    assert scene["dequantization_summand"].view(np.uint32)[2] == 0
    assert (scene["quantized_positions"][:, 1] >> 10 == 0).all()
    assert np.isfinite(scene["dequantization_summand"]).all()
    other = se.export(**cases.planar_mesh(-z))
    assert not cases.buffers_differ(scene, other)


def test_a_single_point():
    scene = se.export(**cases.EDGE_MESHES["one_vertex"]())
    assert (scene["quantized_positions"] == 0).all() and (scene["dequantization_factor"] == 0.0).all()
    assert scene["dequantization_summand"].tolist() == [2.5, 2.5, 2.5] and scene["material_names"] == ["no_material_assigned"]


def test_special_normals():
    """(0, 0, 1) is the centre; z <= 0 folds, also for -0; the sign of a component that is -0 counts as +; the zero
    normal is the centre by this project's rule"""
    scene = se.export(sort_triangles=False, **cases.special_normal_mesh())
    codes = scene["normals_and_tex_coords"][::3, :2]
    assert [tuple(c) for c in codes[:len(cases.SPECIAL_NORMAL_CODES)].tolist()] == cases.SPECIAL_NORMAL_CODES
    assert (codes >= 1).all()


def test_normals_are_folded_in_binary32_and_scaled_in_binary64():
    """Either other choice changes codes of a few thousand random normals (the header says about 4 in 10 000)"""
    normals = np.random.default_rng(5).normal(size=(40000, 3)).astype(np.float32)
    codes = se.encode_normals(normals).astype(np.int64)
    a = np.abs(normals)
    o = normals[:, :2] / ((a[:, 0] + a[:, 1]) + a[:, 2])[:, None]
    s = np.where(o >= 0, np.float32(1), np.float32(-1))
    folded = np.where(normals[:, 2:3] <= 0, (np.float32(1) - np.abs(o[:, ::-1])) * s, o)
    in_binary32 = (folded * np.float32(32767.0) + np.float32(32768.5)).astype(np.uint16).astype(np.int64)
    assert 0 < (in_binary32 != codes).sum() < 400 and np.abs(in_binary32 - codes).max() == 1


def test_special_tex_coords():
    scene = se.export(sort_triangles=False, **cases.special_tex_coord_mesh())
    codes = scene["normals_and_tex_coords"][:, 2:].reshape(-1, 3, 2)
    assert codes[:len(cases.SPECIAL_TEX_COORD_CODES)].tolist() == [[list(c) for c in t] for t in cases.SPECIAL_TEX_COORD_CODES]


def test_triangles_of_equal_code_keep_input_order():
    mesh = cases.tied_mesh()
    codes = se.morton_codes(mesh["positions"], mesh["indices"])
    assert np.unique(codes).size <= 50
    scene = se.export(**mesh)
    # the copies of a triangle carry the material indices 0, 1, 2 in input order
    if np.unique(codes).size == 50:
        assert scene["material_indices"].reshape(-1, 3).tolist() == [[0, 1, 2]] * 50
    order = np.argsort(codes, kind="stable")
    assert np.array_equal(scene["material_indices"], mesh["material_indices"][order])
    plain = se.export(sort_triangles=False, **mesh)
    assert np.array_equal(scene["normals_and_tex_coords"].reshape(-1, 12), plain["normals_and_tex_coords"].reshape(-1, 12)[order])


def test_indexed_input_equals_the_triangle_list():
    mesh = cases.without_unused_vertices(cases.random_mesh(40, 61, seed=11))
    for sort_triangles in (False, True):
        indexed, listed = se.export(sort_triangles=sort_triangles, **mesh), se.export(sort_triangles=sort_triangles, **cases.unindexed(mesh))
        assert not cases.buffers_differ(indexed, listed)
    # (T, 3, 3) arrays are taken as the triangle list
    listed = cases.unindexed(mesh)
    assert not cases.buffers_differ(se.export(**dict(listed, positions=listed["positions"].reshape(-1, 3, 3), normals=listed["normals"].reshape(-1, 3, 3))), se.export(**listed))


def test_unused_vertices_count_for_the_box():
    mesh = dict(cases.random_mesh(40, 61, seed=11))
    far = dict(mesh, positions=np.concatenate([mesh["positions"], np.full((1, 3), 100.0, np.float32)]), normals=np.concatenate([mesh["normals"], np.ones((1, 3), np.float32)]))
    assert (se.export(**far)["dequantization_factor"] > se.export(**mesh)["dequantization_factor"]).all()


def test_material_names():
    assert [se.substitute_material_name(n) for n in ("brick.001", "glass.DoubleSided", "floor", "a.12", "a.1234", "x.DoubleSided.007", ".DoubleSided.DoubleSided", ".Double.DoubleSidedSided", "b.00a")] \
        == ["brick", "glass", "floor", "a.12", "a.1234", "x", "", ".DoubleSided", "b.00a"]


def test_invalid_input_is_refused():
    mesh = cases.random_mesh(40, 61, seed=11)
    bad_index = mesh["indices"].copy()
    bad_index[60, 2] = 40
    bad_material = mesh["material_indices"].copy()
    bad_material[7] = 3
    nan_position = mesh["positions"].copy()
    nan_position[39, 1] = np.nan
    infinite_uv = mesh["tex_coords"].copy()
    infinite_uv[60, 2, 1] = np.inf
    for change in (dict(indices=bad_index), dict(material_indices=bad_material), dict(positions=nan_position), dict(tex_coords=infinite_uv),
                   dict(material_names=()), dict(material_names=("m",) * 257), dict(indices=np.zeros((0, 3), np.uint32), tex_coords=None, material_indices=None)):
        with pytest.raises(ValueError):
            se.export(**dict(mesh, **change))


def test_export_scene_needs_a_device():
    """There is no host build of the exporter: 1, the struct zeroed"""
    lib = capi.load()
    source, keepalive = se.export_source(**cases.random_mesh(40, 61, seed=11))
    scene = capi.ExportedScene()
    scene.triangle_count = 5
    assert lib.export_scene(C.byref(scene), None, C.byref(source), 1) == 1
    assert bytes(scene) == bytes(C.sizeof(scene))
    assert lib.write_exported_scene(C.byref(scene), b"/nonexistent/scene.vks") == 1
    lib.free_exported_scene(C.byref(scene))


OBJ = """# a quad, a triangle given by negative indices, two materials, a face without vn / vt
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0.5
vn 0 0 1
vt 0 0
vt 1 0
vt 1 1
vt 0 1
usemtl wall.001
f 1/1/1 2/2/1 3/3/1 4/4/1
usemtl glass
f -4/-4/-1 -3/-3/-1 -1/-1/-1
usemtl wall.001
f 1 2 3
"""


def test_read_obj(tmp_path):
    path = tmp_path / "mesh.obj"
    path.write_text(OBJ)
    mesh = se.read_obj(str(path))
    assert mesh["material_names"] == ["wall.001", "glass"] and mesh["material_indices"].tolist() == [0, 0, 1, 0]
    v = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0.5)], np.float32)
    # the quad is fanned from its first corner; -4, -3, -1 are vertices 1, 2, 4
    assert np.array_equal(mesh["positions"].reshape(4, 3, 3), v[[(0, 1, 2), (0, 2, 3), (0, 1, 3), (0, 1, 2)]])
    uv = np.array([(0, 0), (1, 0), (1, 1), (0, 1)], np.float32)
    assert np.array_equal(mesh["tex_coords"][:3], uv[[(0, 1, 2), (0, 2, 3), (0, 1, 3)]]) and (mesh["tex_coords"][3] == 0).all()
    assert (mesh["normals"][:9] == (0, 0, 1)).all()
    # the face without vn takes its geometric normal
    assert np.allclose(mesh["normals"][9:], (0, 0, 1)) and mesh["normals"].dtype == np.float32
    scene = se.export(**mesh)
    assert scene["material_names"] == ["wall", "glass"] and scene["material_indices"].shape == (4,)
    # without usemtl and without faces
    bare = tmp_path / "bare.obj"
    bare.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    assert se.read_obj(str(bare))["material_names"] == ["no_material_assigned"]
    bare.write_text("v 0 0 0\nf 1 2 5\n")
    with pytest.raises(ValueError):
        se.read_obj(str(bare))


def test_the_writer_and_the_loader(golden, tmp_path):
    """write_exported_scene() writes the bytes of the restatement - for the golden mesh the add-on's file -, and the
    unchanged host loader reads the buffers back"""
    lib = capi.load()
    mesh = cases.golden_mesh(golden, "medium")
    exported = se.export(**mesh)
    scene, keepalive = se.exported_scene(exported)
    path = str(tmp_path / "scene.vks")
    assert lib.write_exported_scene(C.byref(scene), path.encode()) == 0
    assert open(path, "rb").read() == se.vks_bytes(exported) == golden["medium_file_sorted"].tobytes()
    assert lib.write_exported_scene(C.byref(scene), str(tmp_path / "missing" / "scene.vks").encode()) == 1
    hs = renderer.HostScene()
    hs.load_scene(path, None)
    T = hs.app.scene.mesh.triangle_count
    assert T == 3000 and hs.app.scene.materials.material_count == 3
    assert [hs.app.scene.materials.material_names[i] for i in range(3)] == [b"brick", b"glass", b"floor"]
    inputs = {"quantized_positions": np.ctypeslib.as_array(hs.app.scene.mesh.host_positions, (T * 3, 2)),
              "normals_and_tex_coords": np.ctypeslib.as_array(hs.app.scene.mesh.host_normals_and_tex_coords, (T * 3, 4)),
              "material_indices": np.ctypeslib.as_array(hs.app.scene.mesh.host_material_indices, (T,)),
              "dequantization_factor": np.array(hs.app.scene.mesh.dequantization_factor[:], np.float32),
              "dequantization_summand": np.array(hs.app.scene.mesh.dequantization_summand[:], np.float32),
              "material_names": exported["material_names"]}
    assert not cases.buffers_differ(inputs, exported)
    hs.close()
    # dequantised positions are within a cell of the input: half a cell from the truncation, and the cell number, up to
    # 2^21, is computed in binary32 (roundings of qf, qo, the product and the sum, 2^-3 cells at most each)
    q = exported["quantized_positions"].astype(np.uint64)
    cells = np.stack([q[:, 0] & 0x1FFFFF, ((q[:, 0] >> 21) | (q[:, 1] << 11)) & 0x1FFFFF, q[:, 1] >> 10], -1).astype(np.float64)
    decoded = cells * exported["dequantization_factor"] + exported["dequantization_summand"]
    order = np.argsort(se.morton_codes(mesh["positions"], mesh["indices"]), kind="stable")
    original = mesh["positions"][mesh["indices"][order].reshape(-1)]
    assert np.abs(decoded - original).max() <= exported["dequantization_factor"].max()
