"""TEST INFRASTRUCTURE.  Generates tests/golden/scene_export.npz from the reference's Blender add-on
(tools/io_export_vulkan_blender28.py), loaded at generation time under a stub `bpy` module: its Scene is replaced by an
object that hands over one prepared Mesh, and its export_scene() writes the file.  For each mesh the input arrays (ours)
and the bytes of the add-on's file, sorted and unsorted, are stored.  Only data is stored: nothing of the add-on's text.
The sorted meshes have no two equal Morton codes (asserted): among equal codes the add-on's order depends on the numpy
build, without them its file is unique.
Run from the repository root:
    python tests/golden/make_scene_export.py [--reference /root/reference]"""
import argparse
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from vulkan_renderer_amd import scene_export  # noqa: E402

MATERIAL_NAMES = ["brick.001", "glass.DoubleSided", "floor"]
# name: (vertex count, triangle count)
MESHES = {"small": (40, 61), "medium": (1500, 3000)}
FIRST_SEED = 20


def make_mesh(seed, vertex_count, triangle_count):
    """Seeded Gaussian vertices and normals, Gaussian uvs times 2.5, random index triples"""
    rng = np.random.default_rng(seed)
    return {"positions": rng.normal(size=(vertex_count, 3)).astype(np.float32),
            "normals": rng.normal(size=(vertex_count, 3)).astype(np.float32),
            "indices": rng.integers(0, vertex_count, (triangle_count, 3)).astype(np.uint32),
            "tex_coords": (rng.normal(size=(triangle_count, 3, 2)) * 2.5).astype(np.float32),
            "material_indices": rng.integers(0, len(MATERIAL_NAMES), triangle_count).astype(np.uint8)}


def mesh_without_equal_codes(vertex_count, triangle_count):
    for seed in range(FIRST_SEED, FIRST_SEED + 100):
        mesh = make_mesh(seed, vertex_count, triangle_count)
        codes = scene_export.morton_codes(mesh["positions"], mesh["indices"])
        if np.unique(codes).size == triangle_count:
            return seed, mesh
    raise RuntimeError("no seed without equal Morton codes")


def load_addon(reference):
    """The add-on as a module; what it asks of Blender at import time is a base class and property declarations"""
    bpy = types.ModuleType("bpy")
    declaration = lambda *args, **kwargs: None
    bpy.types = types.SimpleNamespace(Operator=type("Operator", (), {}))
    bpy.props = types.SimpleNamespace(StringProperty=declaration, BoolProperty=declaration, FloatProperty=declaration)
    sys.modules["bpy"] = bpy
    spec = importlib.util.spec_from_file_location("vks_addon", os.path.join(reference, "tools", "io_export_vulkan_blender28.py"))
    addon = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(addon)
    return addon


def addon_file(addon, mesh, sort_triangles, directory):
    """The bytes export_scene() of the add-on writes for the mesh"""
    prepared = addon.Mesh()
    triangle_count = mesh["indices"].shape[0]
    prepared.primitive_vertex_count = np.full(triangle_count, 3, np.uint32)
    prepared.primitive_vertex_indices = mesh["indices"].reshape(-1).copy()
    prepared.primitive_material_index = mesh["material_indices"].astype(np.uint32)
    prepared.primitive_vertex_uv = mesh["tex_coords"].reshape(-1, 2).copy()
    prepared.vertex_position = mesh["positions"].copy()
    prepared.vertex_normal = mesh["normals"].copy()
    prepared.slot_material_name = list(MATERIAL_NAMES)

    class OneMeshScene:
        def __init__(self, *_arguments):
            self.mesh_list = [prepared]

        def get_merged_mesh(self):
            return prepared

    addon.Scene = OneMeshScene
    path = os.path.join(directory, "scene.vks")
    addon.export_scene(None, path, False, False, None, sort_triangles)
    with open(path, "rb") as file:
        return np.frombuffer(file.read(), np.uint8)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--reference", default="/root/reference")
    arguments = parser.parse_args()
    addon = load_addon(arguments.reference)
    stored = {"material_names": np.array(MATERIAL_NAMES)}
    with tempfile.TemporaryDirectory() as directory:
        for name, (vertex_count, triangle_count) in MESHES.items():
            seed, mesh = mesh_without_equal_codes(vertex_count, triangle_count)
            stored[name + "_seed"] = np.array(seed)
            for key, value in mesh.items():
                stored["%s_%s" % (name, key)] = value
            for sort_triangles in (False, True):
                stored["%s_file_%s" % (name, "sorted" if sort_triangles else "unsorted")] = addon_file(addon, mesh, sort_triangles, directory)
    path = os.path.join(ROOT, "tests", "golden", "scene_export.npz")
    np.savez_compressed(path, **stored)
    print("wrote %s: %d bytes, numpy %s" % (path, os.path.getsize(path), np.__version__))


if __name__ == "__main__":
    main()
