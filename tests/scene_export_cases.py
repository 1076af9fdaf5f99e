"""Meshes shared by tests/test_scene_export.py (the numpy restatement of include/vkr_scene_export.h) and
tests/test_gpu_scene_export.py (the device): seeded random meshes, and the inputs for which the add-on leaves the result
open or divides by zero.  Each mesh is a dict of keyword arguments of scene_export.export() and Renderer.export_scene()."""
import functools

import numpy as np

MATERIAL_NAMES = ("brick.001", "glass.DoubleSided", "floor")


@functools.lru_cache(maxsize=None)
def random_mesh(vertex_count, triangle_count, seed=7):
    """Gaussian vertices and normals, Gaussian uvs times 2.5, random index triples, as tests/golden/make_scene_export.py
    makes them"""
    rng = np.random.default_rng(seed)
    return {"positions": rng.normal(size=(vertex_count, 3)).astype(np.float32),
            "normals": rng.normal(size=(vertex_count, 3)).astype(np.float32),
            "indices": rng.integers(0, vertex_count, (triangle_count, 3)).astype(np.uint32),
            "tex_coords": (rng.normal(size=(triangle_count, 3, 2)) * 2.5).astype(np.float32),
            "material_indices": rng.integers(0, len(MATERIAL_NAMES), triangle_count).astype(np.uint8),
            "material_names": MATERIAL_NAMES}


def golden_mesh(golden, name):
    mesh = {key: golden["%s_%s" % (name, key)] for key in ("positions", "normals", "indices", "tex_coords", "material_indices")}
    mesh["material_names"] = tuple(str(n) for n in golden["material_names"])
    return mesh


def planar_mesh(z):
    """Every vertex at height z (0.0 or -0.0): the box is flat along z"""
    mesh = dict(random_mesh(40, 61, seed=11))
    mesh["positions"] = mesh["positions"].copy()
    mesh["positions"][:, 2] = z
    return mesh


SPECIAL_NORMALS = np.array([(0, 0, 1), (0, 0, -1), (1, 0, 0), (-1, 0, 0), (-0.0, 0.5, -0.0), (0, 0, 0), (0, -0.0, 2), (1e-30, -1e-30, -1e-38),
                            (3e38, 3e38, 3e38)], np.float32)
# (the codes of the first six by hand: see test_special_normals)
SPECIAL_NORMAL_CODES = [(32768, 32768), (65535, 65535), (65535, 32768), (1, 32768), (32768, 65535), (32768, 32768)]


def special_normal_mesh():
    """One triangle per special normal, on vertices of a random mesh"""
    n = len(SPECIAL_NORMALS)
    mesh = dict(random_mesh(3 * n, n, seed=12))
    mesh["normals"] = np.repeat(SPECIAL_NORMALS, 3, axis=0)
    mesh["indices"] = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    return mesh


SPECIAL_TEX_COORDS = np.array([
    [(0.0, 0.0), (9.5, 0.0), (0.0, 20.0)],            # more than eight repetitions: clamped
    [(-1.25, -0.5), (-0.25, -0.5), (-1.25, 0.25)],    # negative: shifted by floor(-1.25) = -2 and floor(-0.5) = -1
    [(3.0, 3.0), (4.0, 3.0), (3.0, 4.0)],             # exactly integral
    [(7.99999, 0.0), (8.0, 0.0), (0.0, 8.00001)],     # next to the clamp
    [(-0.0, 0.0), (1e-6, -1e-6), (0.5, 0.5)],         # -0 and a minimum just below zero
], np.float32)
SPECIAL_TEX_COORD_CODES = [[(0, 0), (65535, 0), (0, 65535)], [(6144, 4096), (14336, 4096), (6144, 10240)], [(0, 0), (8192, 0), (0, 8192)]]


def special_tex_coord_mesh():
    n = len(SPECIAL_TEX_COORDS)
    mesh = dict(random_mesh(20, n, seed=13))
    mesh["tex_coords"] = SPECIAL_TEX_COORDS
    return mesh


def tied_mesh():
    """Triangles with equal Morton codes: every triangle of a small random mesh three times, the copies (with uvs and
    materials of their own) apart from each other in the input.  Sorted, the copies are neighbours in input order."""
    base = random_mesh(30, 50, seed=14)
    rng = np.random.default_rng(15)
    mesh = dict(base)
    mesh["indices"] = np.concatenate([base["indices"]] * 3)
    mesh["tex_coords"] = (rng.normal(size=(150, 3, 2)) * 2.5).astype(np.float32)
    mesh["material_indices"] = (np.arange(150) // 50).astype(np.uint8)
    return mesh


def unindexed(mesh):
    """The same mesh as a triangle list"""
    corners = mesh["indices"].reshape(-1)
    return dict(mesh, positions=mesh["positions"][corners], normals=mesh["normals"][corners], indices=None)


def without_unused_vertices(mesh):
    """(unused vertices count for the box: indexed and un-indexed exports agree only without them)"""
    used = np.unique(mesh["indices"])
    return dict(mesh, positions=mesh["positions"][used], normals=mesh["normals"][used], indices=np.searchsorted(used, mesh["indices"]).astype(np.uint32))


EDGE_MESHES = {
    "planar": lambda: planar_mesh(0.0),
    "planar_negative_zero": lambda: planar_mesh(-0.0),
    "special_normals": special_normal_mesh,
    "special_tex_coords": special_tex_coord_mesh,
    "tied": tied_mesh,
    "unindexed": lambda: unindexed(random_mesh(40, 61, seed=11)),
    "one_vertex": lambda: dict(positions=np.full((1, 3), 2.5, np.float32), normals=np.array([[0.0, 1.0, 1.0]], np.float32), indices=np.zeros((2, 3), np.uint32)),
    "defaults": lambda: dict(positions=random_mesh(40, 61, seed=11)["positions"][:39], normals=random_mesh(40, 61, seed=11)["normals"][:39]),
}


def buffers_differ(got, expected):
    """Names of the buffers that differ, with the number of differing bytes"""
    out = {}
    for key in ("quantized_positions", "normals_and_tex_coords", "material_indices", "dequantization_factor", "dequantization_summand"):
        a, b = np.ascontiguousarray(got[key]), np.ascontiguousarray(expected[key])
        if a.dtype != b.dtype or a.shape != b.shape:
            out[key] = "dtype / shape %s %s against %s %s" % (a.dtype, a.shape, b.dtype, b.shape)
        elif a.tobytes() != b.tobytes():
            out[key] = int((a.view(np.uint8) != b.view(np.uint8)).sum())
    if list(got["material_names"]) != list(expected["material_names"]):
        out["material_names"] = got["material_names"]
    return out
