"""The host side of moving geometry (include/vkr_scene_update.h, vulkan_renderer_amd/scene_update.py) without a GPU: the
position codes against the de-quantisation of the ray queries, the slab boxes of split triangles, the numpy restatement
of the refit on a tree small enough to work out by hand, and the struct mirrors."""
import ctypes as C

import numpy as np
import pytest

import scene_update_cases as cases
from vulkan_renderer_amd import capi, ray_queries, scene_update

L = scene_update.LEAF_BIT


def test_codes_round_trip_through_the_words_and_the_dequantisation():
    rng = np.random.default_rng(5)
    codes = rng.integers(0, 1 << 21, (4098, 3)).astype(np.uint32)
    codes[:4] = [[0, 0, 0], [scene_update.CODE_MAX] * 3, [0, scene_update.CODE_MAX, 0x155555], [0x0AAAAA, 0x7FF, 0x800]]
    words = scene_update.pack_positions(codes)
    assert words.dtype == np.uint32 and words.shape == (4098, 2) and not (words[:, 1] >> 31).any()
    assert np.array_equal(scene_update.unpack_positions(words), codes)
    # the words mean what the loaders take them to mean, to the bit
    factor, summand = np.array([3.1e-6, 7.7e-6, 1.3e-6], np.float32), np.array([-8.0, -3.5, 0.25], np.float32)
    vertices = ray_queries.dequantize(words, factor, summand).reshape(-1, 3)
    assert np.array_equal(vertices.view(np.uint32), (codes.astype(np.float32) * factor + summand).view(np.uint32))
    # ... and quantize() finds the code of every de-quantised vertex again
    again, clamped = scene_update.quantize(vertices, factor, summand)
    assert not clamped.any() and np.array_equal(again, codes)
    # half a cell outside the outermost cell centres is still inside the box; a whole cell is not
    s, f = summand.astype(np.float64), factor.astype(np.float64)
    edge = np.array([s - 0.5 * f, s + (scene_update.CODE_MAX + 0.5) * f, s - 1.0 * f, s + (scene_update.CODE_MAX + 1.0) * f])
    snapped, clamped = scene_update.quantize(edge, factor, summand)
    assert clamped.tolist() == [False, False, True, True]
    assert np.array_equal(snapped, [[0] * 3, [scene_update.CODE_MAX] * 3, [0] * 3, [scene_update.CODE_MAX] * 3])
    with pytest.raises(ValueError):
        scene_update.pack_positions([[1 << 21, 0, 0]])


def test_rewriting_the_position_block_of_a_scene_file(tmp_path):
    dataset = cases.write_case(tmp_path / "rest", 17)
    words = cases.read_vks_positions(dataset["scene"])
    triangle_count, factor, summand, _ = cases.read_vks_header(dataset["scene"])
    assert triangle_count == 17 and words.shape == (51, 2)
    # the file holds the mesh at rest, in the order of MESHES (half a cell is as far as quantisation moves a vertex)
    assert np.abs(ray_queries.dequantize(words, factor, summand) - cases.MESHES[17]).max() <= 0.5 * float(factor.max()) * 1.001 + 1.0e-6
    moved = cases.quantized(dataset, cases.motion(17, 1))
    assert (moved != words).any() and np.array_equal(moved[:6], words[:6])
    target = str(tmp_path / "moved.vks")
    cases.rewrite_vks_positions(dataset["scene"], target, moved)
    assert np.array_equal(cases.read_vks_positions(target), moved)
    with open(dataset["scene"], "rb") as a, open(target, "rb") as b:
        before, after = a.read(), b.read()
    offset = cases.read_vks_header(target)[3]
    assert len(before) == len(after) and before[:offset] == after[:offset] and before[offset + moved.nbytes:] == after[offset + moved.nbytes:]


@pytest.mark.parametrize("name", sorted(cases.MESHES, key=str))
def test_no_motion_leaves_the_box_of_its_file(tmp_path, name):
    dataset = cases.write_case(tmp_path, name)
    rest = cases.read_vks_positions(dataset["scene"])
    for step in range(1, 4):
        words = cases.quantized(dataset, cases.motion(name, step))
        fixed = 3 * cases.FIXED[name]
        # (the occluder goes back and forth)
        assert np.array_equal(words[:fixed], rest[:fixed]) and ((words[fixed:] != rest[fixed:]).any() or (name == "occluder" and step == 2))


def test_the_slabs_of_a_triangle_cover_it():
    """Every point of a triangle lies in the box of one of its fragments, for 1 to 16 slabs along every axis: what lets a
    leaf per fragment stand for the triangle.  The points are float64 combinations of the float32 vertices and the planes
    between the slabs are rounded, so a point may miss its box by the rounding of a coordinate: 2^-22 of the largest one."""
    rng = np.random.default_rng(11)
    weights = rng.dirichlet([1.0, 1.0, 1.0], 200)
    weights = np.concatenate([weights, np.eye(3), [[0.5, 0.5, 0.0], [0.0, 0.5, 0.5], [0.5, 0.0, 0.5]]], 0)
    for _ in range(6):
        triangle = (rng.uniform(-8.0, 8.0, (1, 3)) + rng.uniform(-1.0, 1.0, (3, 3)) * rng.uniform(0.01, 3.0, 3)).astype(np.float32)
        lo, hi = triangle.min(axis=0), triangle.max(axis=0)
        points = weights @ triangle.astype(np.float64)
        slack = 2.0 ** -22 * float(np.abs(triangle).max())
        for axis in range(3):
            for count in range(1, 17):
                boxes = [scene_update.slab_box(triangle, lo, hi, axis, j, count) for j in range(count)] if count > 1 else [(lo, hi)]
                inside = np.zeros(len(points), bool)
                for flo, fhi in boxes:
                    assert (flo >= lo).all() and (fhi <= hi).all() and (flo <= fhi).all()
                    inside |= ((points >= flo - slack) & (points <= fhi + slack)).all(axis=1)
                assert inside.all(), (axis, count, int((~inside).sum()))
                # the slabs tile the triangle's box along the axis: each begins where the one before it ends
                if count > 1:
                    assert boxes[0][0][axis] == lo[axis] and boxes[-1][1][axis] == hi[axis]


def packed(lo, hi):
    return [l | (h << 16) for l, h in zip(lo, hi)]


def test_refit_reference_on_a_tree_worked_out_by_hand():
    """Four triangles, the seven nodes of their binary tree in depth-first order and a wide form of two nodes.  Factor 2^-10
    and summand 0 make the vertices exact; the padding is 2e-6 * 2048.  The box of the mesh is [1, 8]^2 x [0, 4] plus the
    padding, a cell of the grid is that over 32765 and the grid begins one cell below.  The expected cells were worked out
    in exact rational arithmetic: with the margin of 0.05 cells no bound comes closer than 0.16 cells to a whole number,
    so float32 cannot round it to the other side."""
    factor, summand = np.full(3, 2.0 ** -10, np.float32), np.zeros(3, np.float32)
    codes = np.array([[[1024, 1024, 0], [3072, 1024, 0], [1024, 2048, 1024]],
                      [[4096, 1024, 0], [5120, 3072, 0], [4096, 2048, 2048]],
                      [[1024, 5120, 0], [2048, 6144, 0], [1024, 6144, 3072]],
                      [[7168, 7168, 1024], [8192, 7168, 1024], [8192, 8192, 4096]]], np.uint32)
    words = scene_update.pack_positions(codes)
    nodes = np.zeros((7, 4), np.uint32)
    nodes[:, :3] = 0xDEADBEEF
    # node 0 (1 (2: leaf 0, 3: leaf 1), 4 (5: leaf 2, 6: leaf 3)): an inner node links to the node behind its subtree
    nodes[:, 3] = [7, 4, L | 0, L | 1, 7, L | 2, L | 3]
    wide = np.full((2, 16), 0xDEADBEEF, np.uint32)
    wide[0, 3::4], wide[1, 2::4], wide[1, 3::4] = scene_update.WIDE_EMPTY_BOX, scene_update.WIDE_EMPTY_BOX, scene_update.WIDE_EMPTY_BOX
    wide[0, 12:] = [L | 0, 1, L | 1, scene_update.WIDE_EMPTY]
    wide[1, 12:] = [L | 2, L | 3, scene_update.WIDE_EMPTY, scene_update.WIDE_EMPTY]
    triangles = np.full((12, 4), 7.0, np.float32)
    # (the leaf slots hold the triangles in another order than the file)
    order = np.array([2, 0, 3, 1], np.uint32)
    triangles[0::3, 3] = order.view(np.float32)
    inverse = np.argsort(order)
    nodes[[2, 3, 5, 6], 3] = L | inverse.astype(np.uint32)
    wide[0, 12], wide[0, 14], wide[1, 12], wide[1, 13] = nodes[2, 3], nodes[3, 3], nodes[5, 3], nodes[6, 3]
    tree = {"nodes": nodes, "wide_nodes": wide, "triangle_vertices": triangles, "leaf_fragments": np.ones(4, np.uint32),
            "grid_origin": np.zeros(3, np.float32), "grid_inverse_cell": np.ones(3, np.float32)}
    out = scene_update.refit_reference(tree, words, factor, summand)
    leaf = [packed((0, 0, 0), (9390, 4715, 8243)), packed((14026, 0, 0), (18741, 9390, 16418)),
            packed((0, 18701, 0), (4715, 23416, 24592)), packed((28052, 28052, 8175), (32767, 32767, 32767))]
    left, right, root = packed((0, 0, 0), (18741, 9390, 16418)), packed((0, 18701, 0), (32767, 32767, 32767)), packed((0, 0, 0), (32767, 32767, 32767))
    assert out["nodes"][:, :3].tolist() == [root, left, leaf[0], leaf[1], right, leaf[2], leaf[3]]
    assert np.array_equal(out["nodes"][:, 3], nodes[:, 3])
    empty = [scene_update.WIDE_EMPTY_BOX] * 3
    assert out["wide_nodes"][0].reshape(4, 4).T[:, :3].tolist() == [leaf[0], right, leaf[1], empty]
    assert out["wide_nodes"][1].reshape(4, 4).T[:, :3].tolist() == [leaf[2], leaf[3], empty, empty]
    assert np.array_equal(out["wide_nodes"][:, 12:], wide[:, 12:])
    # vertices of the slots' triangles, w untouched
    assert np.array_equal(out["triangle_vertices"][:, :3].reshape(4, 3, 3), codes[order].astype(np.float32) / 1024.0)
    assert np.array_equal(out["triangle_vertices"][:, 3].view(np.uint32), triangles[:, 3].view(np.uint32))
    # the three sums over the inner nodes 0, 1 and 4
    extents = [(32767, 32767, 32767), (18741, 9390, 16418), (32767, 14066, 32767)]
    assert out["cost_sums"] == [sum(e[a] * e[b] for e in extents) for a, b in ((0, 1), (1, 2), (2, 0))]
    pad = np.float32(2.0e-6) * np.float32(2048.0)
    cell = [(7.0 + 2.0 * float(pad)) / 32765.0, (7.0 + 2.0 * float(pad)) / 32765.0, (4.0 + 2.0 * float(pad)) / 32765.0]
    assert np.allclose(out["grid_inverse_cell"], 1.0 / np.array(cell), rtol=1.0e-6)
    assert np.allclose(out["grid_origin"], np.array([1.0, 1.0, 0.0]) - float(pad) - np.array(cell), rtol=1.0e-6, atol=1.0e-7)
    assert out["cost"] == pytest.approx(sum(s * a * b for s, (a, b) in zip(out["cost_sums"], ((cell[0], cell[1]), (cell[1], cell[2]), (cell[2], cell[0])))), rel=1.0e-6)
    assert scene_update.differences(out, out) == [] and scene_update.differences(tree, out) == ["nodes", "wide_nodes", "triangle_vertices", "grid_origin", "grid_inverse_cell"]


def test_struct_mirrors_of_the_scene_update():
    """the sizes of the new structs and of the grown acceleration_structure_t agree with the library's"""
    lib = capi.load()
    sizes = (C.c_uint64 * 32)()
    count = lib.get_abi_struct_sizes(sizes, 32)
    assert count == len(capi.ABI_STRUCTS)
    by_class = dict(zip(capi.ABI_STRUCTS, sizes))
    assert by_class[capi.SceneUpdateOptions] == C.sizeof(capi.SceneUpdateOptions) == 20
    assert by_class[capi.SceneUpdateReport] == C.sizeof(capi.SceneUpdateReport) == 32
    assert by_class[capi.AccelerationStructure] == C.sizeof(capi.AccelerationStructure)
    assert capi.AccelerationStructure.built_cost.offset + 8 == C.sizeof(capi.AccelerationStructure)
    assert hasattr(lib, "update_scene_geometry")
    assert scene_update.POLICY == {"refit": 0, "rebuild": 1, "auto": 2}


def test_update_scene_geometry_rejects_what_it_cannot_use():
    """the failures that need no device: they are found before anything is touched"""
    lib = capi.load()
    scene, device, report = capi.Scene(), capi.Device(), capi.SceneUpdateReport()
    words = np.zeros((3, 2), np.uint32)
    assert lib.update_scene_geometry(None, C.byref(device), words.ctypes.data, None, None, C.byref(report)) == 1
    assert lib.update_scene_geometry(C.byref(scene), None, words.ctypes.data, None, None, C.byref(report)) == 1
    assert lib.update_scene_geometry(C.byref(scene), C.byref(device), None, None, None, C.byref(report)) == 1
    for options in (capi.SceneUpdateOptions(3, 0, 1, 0, 0.0), capi.SceneUpdateOptions(0, 0, 1, 0, -1.0), capi.SceneUpdateOptions(2, 0, 1, 0, float("nan"))):
        assert lib.update_scene_geometry(C.byref(scene), C.byref(device), words.ctypes.data, None, C.byref(options), C.byref(report)) == 1
