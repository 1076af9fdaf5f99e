"""Host-side driver of the shading pass, written against the C-ABI only.

It plays the role of the reference's startup_application / render_frame
(src/main.c:1896, :2197) for tests and bench.py: load the scene, LTC table and
noise table, specify lights and settings, create the pass, render, read back.
All arithmetic happens inside libvkr_shading.so; if the library or a GPU is
missing, construction fails loudly - there is no CPU fallback."""
import ctypes as C
import math

import numpy as np

from . import capi
from .frame_images import FrameFilter, FrameHistory, FrameStatistics, _address, _DeviceScratch, _hip_runtime  # noqa: F401 (used under this module's name)

STRATEGY = {"diffuse_only": 0, "diffuse_ggx_mis": 1, "diffuse_specular_separately": 2,
            "diffuse_specular_mis": 3, "diffuse_specular_random": 4}
MIS = {"balance": 0, "power": 1, "weighted": 2, "optimal_clamped": 3, "optimal": 4}
TECHNIQUE = {"baseline": 0, "area_turk": 1, "rectangle_solid_angle_urena": 2, "solid_angle_arvo": 3,
             "bilinear_cosine_warp_hart": 6, "bilinear_cosine_warp_clipping_hart": 7,
             "biquadratic_cosine_warp_hart": 8, "biquadratic_cosine_warp_clipping_hart": 9,
             "projected_solid_angle_arvo": 10, "solid_angle": 4, "clipped_solid_angle": 5, "projected_solid_angle": 11,
             "projected_solid_angle_biased": 12}
# noise_type_t (include/vkr_noise_table.h; 3 is noise_type_count)
NOISE = {"white": 0, "blue": 1, "ahmed": 2, "sobol": 4, "owen": 5, "burley_owen": 6, "blue_noise_dithered": 7}
# arithmetic_mode_t; and the math mode of the CPU oracle that evaluates the same operations
ARITHMETIC_MODES = {"libm": 0, "fast": 1, "exact": 2}
ORACLE_MATH_MODE = {"libm": 0, "fast": 0, "exact": 1}
# acceleration_structure_builder_t (include/vkr_scene.h); True selects the default (HIP kernels, binned SAH)
BVH_BUILDER = {False: 0, None: 0, True: 1, "sah_device": 1, "lbvh_device": 2, "sah_host": 3}
BVH_BUILDER_NAME = {0: "none", 1: "binned SAH built by HIP kernels", 2: "Morton-code LBVH built by HIP kernels", 3: "binned SAH built on the host"}


def _enum(table, value):
    return table[value] if isinstance(value, str) else int(value)


class HostScene:
    """Device-less use of the loader surface (parsing, quantisation, constants)."""

    def __init__(self):
        self.lib = capi.load()
        self.app = capi.Application()
        self._device = None
        self._lights_keepalive = None

    # -- loaders -------------------------------------------------------------------
    def _dev(self):
        return C.byref(self.app.device) if self._device else None

    def load_scene(self, path, texture_path=None, acceleration_structure=False):
        rc = self.lib.load_scene(C.byref(self.app.scene), self._dev(), path.encode(),
                                 texture_path.encode() if texture_path else None, BVH_BUILDER[acceleration_structure])
        if rc:
            raise RuntimeError("load_scene failed for %s" % path)

    def load_ltc_table(self, directory, fresnel_count=51):
        # (the fits of an earlier fit_ltc_table() belong to the table that this call replaces)
        self._free_ltc_fits()
        if self.lib.load_ltc_table(C.byref(self.app.ltc_table), self._dev(), directory.encode(), fresnel_count):
            raise RuntimeError("load_ltc_table failed for %s" % directory)

    def load_noise_table(self, noise_type="white", resolution=None):
        t = _enum(NOISE, noise_type)
        res = self.lib.get_default_noise_resolution(t)
        if resolution is not None:
            res = capi.Extent3D(*resolution)
        if self.lib.load_noise_table(C.byref(self.app.noise_table), self._dev(), res, t):
            raise RuntimeError("load_noise_table failed")

    # -- scene specification ---------------------------------------------------------
    def set_camera(self, position, rotation_x, rotation_z, vertical_fov, near=0.05, far=1.0e3):
        cam = self.app.scene_specification.camera
        cam.position_world_space[:] = position
        cam.rotation_x, cam.rotation_z, cam.vertical_fov = rotation_x, rotation_z, vertical_fov
        cam.near, cam.far, cam.speed = near, far, 2.0

    def set_lights(self, lights):
        """lights: list of dicts from synthetic.light_spec()."""
        spec = self.app.scene_specification
        for i in range(spec.polygonal_light_count):
            self.lib.destroy_polygonal_light(C.byref(spec.polygonal_lights[i]))
        array = (capi.PolygonalLight * max(len(lights), 1))()
        for i, l in enumerate(lights):
            light = array[i]
            light.rotation_angles[:] = l["rotation_angles"]
            light.translation[:] = l["translation"]
            light.radiant_flux[:] = l["radiant_flux"]
            light.scaling_x, light.scaling_y = l["scaling"]
            v = np.asarray(l["vertices_plane_space"], np.float32)
            self.lib.set_polygonal_light_vertex_count(C.byref(light), len(v))
            for j in range(len(v)):
                light.vertices_plane_space[4 * j + 0] = float(v[j, 0])
                light.vertices_plane_space[4 * j + 1] = float(v[j, 1])
            light.texturing_technique = {"none": 0, "area": 1, "portal": 2, "ies_profile": 3}.get(l.get("texturing_technique", 0), l.get("texturing_technique", 0))
            if l.get("texture_file_path"):
                # the library frees the path with free(): hand it a malloc'ed copy
                encoded = l["texture_file_path"].encode() + b"\0"
                libc = C.CDLL(None)
                libc.malloc.restype = C.c_void_p
                copy = libc.malloc(len(encoded))
                C.memmove(copy, encoded, len(encoded))
                light.texture_file_path = copy
            self.lib.update_polygonal_light(C.byref(light))
        self._lights_keepalive = array
        spec.polygonal_lights = C.cast(array, C.POINTER(capi.PolygonalLight))
        spec.polygonal_light_count = len(lights)
        # like the reference's update rules (main.c:1831, 1854, 1879): new lights, new light textures
        if self.app.light_textures.texture_count:
            self.lib.destroy_light_textures(C.byref(self.app.light_textures), self._dev())
        if any(l.get("texturing_technique") for l in lights):
            self.create_light_textures()

    def create_light_textures(self):
        if self.lib.create_and_assign_light_textures(C.byref(self.app.light_textures), self._dev(), C.byref(self.app.scene_specification)):
            raise RuntimeError("create_and_assign_light_textures failed")

    def set_settings(self, **kw):
        s = self.app.render_settings
        if "exposure_factor" not in kw and s.exposure_factor == 0.0:
            self.lib.specify_default_render_settings(C.byref(s))
            s.show_polygonal_lights = 0
            s.animate_noise = 0
            s.noise_type = 0
        for key, value in kw.items():
            if key == "sampling_strategies":
                s.sampling_strategies = _enum(STRATEGY, value)
            elif key == "mis_heuristic":
                s.mis_heuristic = _enum(MIS, value)
            elif key in ("polygon_technique", "polygon_sampling_technique"):
                s.polygon_sampling_technique = _enum(TECHNIQUE, value)
            elif key in ("width", "height"):
                pass
            elif key in ("trace_shadow_rays", "show_polygonal_lights", "animate_noise"):
                setattr(s, key, int(bool(value)))
            else:
                setattr(s, key, value)
        if "width" in kw:
            self.app.swapchain.extent.width = kw["width"]
        if "height" in kw:
            self.app.swapchain.extent.height = kw["height"]

    # -- constants --------------------------------------------------------------------
    def constants(self):
        """Byte image of write_constants() as a numpy array."""
        size = self.lib.get_constant_buffer_size(C.byref(self.app))
        buf = np.zeros(size, np.uint8)
        self.lib.write_constants(buf.ctypes.data, C.byref(self.app))
        return buf

    def max_light_vertex_count(self):
        return self.lib.get_max_polygonal_light_vertex_count(C.byref(self.app.scene_specification))

    # -- host views of the loaded data (inputs for the CPU oracle in tests) -------------
    def host_inputs(self, visibility=None):
        app = self.app
        T = app.scene.mesh.triangle_count
        ltc = app.ltc_table
        n = app.noise_table.resolution
        layers, res = ltc.fresnel_count, ltc.roughness_count
        inputs = {
            "constants": self.constants(),
            "light_count": app.scene_specification.polygonal_light_count,
            "max_light_vertex_count": self.max_light_vertex_count(),
            "quantized_positions": np.ctypeslib.as_array(app.scene.mesh.host_positions, (T * 3, 2)).copy(),
            "normals_and_tex_coords": np.ctypeslib.as_array(app.scene.mesh.host_normals_and_tex_coords, (T * 3, 4)).copy(),
            "material_indices": np.ctypeslib.as_array(app.scene.mesh.host_material_indices, (T,)).copy(),
            "material_constants": np.ctypeslib.as_array(app.scene.materials.host_constants, (app.scene.materials.material_count * 8,)).copy(),
            "ltc_rgba": np.ctypeslib.as_array(ltc.host_rgba, (layers, res, res, 4)).copy(),
            "ltc_rg": np.ctypeslib.as_array(ltc.host_rg, (layers, res, res, 2)).copy(),
            "noise": np.ctypeslib.as_array(app.noise_table.host_data, (n.depth, n.height, n.width, 4)).copy(),
            "dequantization_factor": np.array(app.scene.mesh.dequantization_factor[:], np.float32),
            "dequantization_summand": np.array(app.scene.mesh.dequantization_summand[:], np.float32),
        }
        materials = app.scene.materials
        if materials.textured:
            descriptors = np.ctypeslib.as_array(materials.host_texture_descriptors, (materials.material_count * 3, 4)).copy()
            texels = np.ctypeslib.as_array(materials.host_texels, (materials.texel_count, 4)).copy()
            textures = []
            for first, width, height, packed in descriptors:
                count = 0
                w, h = int(width), int(height)
                for _ in range(int(packed) & 0xFFFF):
                    count += w * h
                    w, h = max(w // 2, 1), max(h // 2, 1)
                textures.append({"texels": texels[int(first):int(first) + count] if width else np.zeros((1, 4), np.uint8),
                                 "width": int(width), "height": int(height), "mip_count": int(packed) & 0xFFFF, "srgb": int(packed) >> 16})
            inputs["material_textures"] = textures
        if app.light_textures.texture_count:
            inputs["light_textures"] = self.light_texture_arrays()
        if visibility is not None:
            inputs["visibility"] = np.ascontiguousarray(visibility, np.uint32)
        return inputs

    def light_texture_arrays(self):
        """The loaded light textures as float32 arrays (height, width, 4); None for white."""
        lights = self.app.light_textures
        textures = []
        for i in range(lights.texture_count):
            first, width, height, _ = (int(v) for v in lights.host_descriptors[i])
            textures.append(np.ctypeslib.as_array(lights.host_texels, (lights.texel_count * 4,))[4 * first:4 * (first + width * height)].reshape(height, width, 4).copy() if width else None)
        return textures

    def oracle_settings(self):
        s = self.app.render_settings
        return {"sampling_strategies": s.sampling_strategies, "mis_heuristic": s.mis_heuristic,
                "polygon_technique": s.polygon_sampling_technique, "sample_count": s.sample_count,
                "trace_shadow_rays": bool(s.trace_shadow_rays), "show_polygonal_lights": bool(s.show_polygonal_lights),
                "error_display": int(s.error_display)}

    def _free_ltc_fits(self):
        if getattr(self, "_ltc_fits", None):
            self.lib.free_ltc_fits(self._ltc_fits)
        self._ltc_fits = None

    def close(self):
        app = self.app
        dev = self._dev()
        if getattr(self, "exchange", None) is not None:
            self.destroy_exchange()
        if app.shading_pass.constants_device:
            self.lib.destroy_shading_pass(C.byref(app.shading_pass), dev)
        if app.render_targets.radiance:
            self.lib.destroy_render_targets(C.byref(app.render_targets), dev)
        self.lib.destroy_light_textures(C.byref(app.light_textures), dev)
        self.lib.destroy_scene(C.byref(app.scene), dev)
        self.lib.destroy_ltc_table(C.byref(app.ltc_table), dev)
        self._free_ltc_fits()
        self.lib.destroy_noise_table(C.byref(app.noise_table), dev)
        spec = app.scene_specification
        for i in range(spec.polygonal_light_count):
            self.lib.destroy_polygonal_light(C.byref(spec.polygonal_lights[i]))
        spec.polygonal_light_count = 0
        self._lights_keepalive = None
        if self._device:
            # releases the frame streams that create_hip_device made
            self.lib.destroy_hip_device(C.byref(app.device))
            self._device = None


class Renderer(HostScene):
    """The shading pass on one MI355X."""

    def __init__(self, hip_device=0, stream=None, fast_math=False, inline_rays=False, timing_stride=1, frames_in_flight=1, binary_traversal=False, arithmetic=None, band_count=0):
        super().__init__()
        # the open JPEG, HDR and PNG encoders, and those that encode_jpeg(), encode_hdr() and encode_png() keep
        self._file_encoders, self._file_encoder_cache = [], {}
        # the open FrameStatistics, FrameFilter and FrameHistory objects, and those that filter_frame() and
        # accumulate_history() keep
        self._frame_objects, self._kept_frame_objects = [], {}
        self.binary_traversal = binary_traversal
        self.exchange = None
        self.timing_stride = timing_stride
        self.frames_in_flight = frames_in_flight
        if self.lib.create_hip_device(C.byref(self.app.device), hip_device, stream):
            raise RuntimeError("no usable HIP device: the shading pass has no CPU fallback")
        self._device = True
        # arithmetic_mode_t of include/vkr_shading_pass.h: "libm" (default; equals the oracle's
        # math mode 0 bit for bit), "fast", "exact" (polynomial; equals the oracle's math mode 1)
        self.arithmetic = arithmetic if arithmetic is not None else ("fast" if fast_math else "libm")
        self.fast_math = self.arithmetic == "fast"
        # launches per frame with wavefront rays (0: automatic, include/vkr_shading_pass.h band_count)
        self.band_count = band_count
        self.inline_rays = inline_rays

    def sample_texture(self, texture, inputs, arithmetic=None):
        """The device's material texture sampler (evaluate_device_texture_sampler) on one texture - a dict with "texels"
        (uint8, all levels, RGBA8), "width", "height", "mip_count", "srgb", as host_inputs() lists them - for inputs (n, 6):
        uv, duv_dx, duv_dy.  -> (n, 4) float32, by the kernel of this renderer's arithmetic mode or the named one."""
        texels = np.ascontiguousarray(texture["texels"], np.uint8)
        inputs = np.ascontiguousarray(inputs, np.float32).reshape(-1, 6)
        out = np.zeros((inputs.shape[0], 4), np.float32)
        fp = C.POINTER(C.c_float)
        if self.lib.evaluate_device_texture_sampler(self._dev(), ARITHMETIC_MODES[arithmetic or self.arithmetic], texels.ctypes.data,
                                                    int(texture["width"]), int(texture["height"]), int(texture["mip_count"]), int(texture["srgb"]),
                                                    inputs.ctypes.data_as(fp), out.ctypes.data_as(fp), inputs.shape[0]):
            raise RuntimeError("evaluate_device_texture_sampler failed")
        return out

    def create_targets(self):
        if self.app.render_targets.radiance:
            self.lib.destroy_render_targets(C.byref(self.app.render_targets), self._dev())
        if self.lib.create_render_targets(C.byref(self.app.render_targets), self._dev(), C.byref(self.app.swapchain)):
            raise RuntimeError("create_render_targets failed")

    def create_pass(self):
        if self.app.shading_pass.constants_device:
            self.lib.destroy_shading_pass(C.byref(self.app.shading_pass), self._dev())
        self.app.shading_pass.arithmetic_mode = ARITHMETIC_MODES[self.arithmetic]
        self.app.shading_pass.band_count = int(self.band_count)
        self.app.shading_pass.inline_rays = int(self.inline_rays)
        self.app.shading_pass.timing_stride = int(self.timing_stride)
        self.app.shading_pass.frames_in_flight = int(self.frames_in_flight)
        self.app.shading_pass.binary_traversal = int(self.binary_traversal)
        if self.lib.create_shading_pass(C.byref(self.app.shading_pass), C.byref(self.app)):
            raise RuntimeError("create_shading_pass failed")

    def set_tiles(self, tile_size=16, rank=0, rank_count=1, slab_layout=False):
        t = self.app.tile_schedule
        t.tile_size, t.rank, t.rank_count, t.slab_layout = tile_size, rank, rank_count, int(slab_layout)

    def generate_noise_table(self, noise_type, resolution=None, seed=0, rounds=None):
        """Replaces the noise table by one generated on the device (include/vkr_noise_table.h generate_noise_table):
        "blue", "sobol", "owen", "burley_owen" or "blue_noise_dithered" (generate_dithered_noise_table, annealed for
        `rounds` rounds; None: get_default_dithered_round_count); resolution None: the default of the type.  Returns the
        milliseconds the call took (allocation, kernels and read-back).  Frames in flight are finished first: they read
        the old table."""
        import time
        t = _enum(NOISE, noise_type)
        dithered = t == NOISE["blue_noise_dithered"]
        if rounds is not None and not dithered:
            raise ValueError("only the blue_noise_dithered table is generated in rounds")
        if self.app.shading_pass.constants_device:
            self.finish_frames()
            self.sync()
        res = self.lib.get_default_noise_resolution(t) if resolution is None else capi.Extent3D(*resolution)
        if dithered and rounds is None:
            rounds = self.lib.get_default_dithered_round_count(res)
        self.lib.destroy_noise_table(C.byref(self.app.noise_table), self._dev())
        start = time.perf_counter()
        if dithered:
            if not 0 <= int(rounds) <= 0xFFFFFFFF or self.lib.generate_dithered_noise_table(C.byref(self.app.noise_table), self._dev(), res, int(seed) & 0xFFFFFFFF, int(rounds)):
                raise RuntimeError("generate_dithered_noise_table failed")
        elif self.lib.generate_noise_table(C.byref(self.app.noise_table), self._dev(), res, t, int(seed) & 0xFFFFFFFF):
            raise RuntimeError("generate_noise_table failed")
        return (time.perf_counter() - start) * 1.0e3

    def write_noise_table(self, noise_type, data_root=None, path=None):
        """Writes the table as a blob: to `path`, or under the reference's file name below data_root (default: the
        working directory), where load_noise_table() looks for it.  Returns the path."""
        import os
        t = _enum(NOISE, noise_type)
        cwd = os.getcwd()
        if path is None and data_root is not None:
            os.makedirs(data_root, exist_ok=True)
            os.chdir(data_root)
        try:
            if self.lib.write_noise_table(C.byref(self.app.noise_table), t, path.encode() if path else None):
                raise RuntimeError("write_noise_table failed")
        finally:
            os.chdir(cwd)
        if path is not None:
            return path
        from . import noise_tables
        n = self.app.noise_table.resolution
        names = {v: k for k, v in NOISE.items()}
        return os.path.join(data_root or cwd, noise_tables.file_name(names[t], (n.width, n.height, n.depth)))

    def convert_texture(self, image, vk_format, path=None):
        """Converts an image (height x width x channels; float32 for the formats 90, 97, 106 and 109, uint8 for 37, 43,
        131, 132 and 141) to a texture on the device (include/vkr_texture_conversion.h convert_texture) and writes it to
        `path` as *.vkt if one is given.  Returns ([(width, height)], [bytes]) of the levels, largest first.  The call
        runs on the device's stream behind whatever is queued there; it touches nothing a frame in flight reads."""
        from . import texture_conversion
        image = np.ascontiguousarray(image, np.float32 if texture_conversion.takes_float(vk_format) else np.uint8)
        if image.ndim != 3:
            raise ValueError("convert_texture takes a height x width x channels array")
        texture = capi.ConvertedTexture()
        if self.lib.convert_texture(C.byref(texture), self._dev(), image.ctypes.data, image.shape[1], image.shape[0], image.shape[2], int(vk_format)):
            raise RuntimeError("convert_texture failed")
        try:
            if path is not None and self.lib.write_converted_texture(C.byref(texture), str(path).encode()):
                raise RuntimeError("write_converted_texture failed for %s" % path)
            payload = C.string_at(texture.payload, texture.payload_size)
            extents = [(texture.width >> i, texture.height >> i) for i in range(texture.mipmap_count)]
            payloads = [payload[texture.mipmap_offsets[i]:texture.mipmap_offsets[i] + texture.mipmap_sizes[i]] for i in range(texture.mipmap_count)]
        finally:
            self.lib.free_converted_texture(C.byref(texture))
        return extents, payloads

    def export_scene(self, positions, normals, indices=None, tex_coords=None, material_indices=None, material_names=("no_material_assigned",), sort_triangles=True, path=None):
        """Exports a triangle mesh to a scene on the device (include/vkr_scene_export.h export_scene) and writes it to
        `path` as *.vks if one is given.  positions, normals: (V, 3); indices: (T, 3), or None for the triangle list;
        tex_coords: (T, 3, 2) per corner or None; material_indices: (T,) or None.  Returns the buffers as they are stored
        in the file, under the names synthetic.write_vks() gives them, and the substituted material names.  The call runs
        on the device's stream behind whatever is queued there; it touches nothing a frame in flight reads."""
        from . import scene_export
        source, keepalive = scene_export.export_source(positions, normals, indices, tex_coords, material_indices, material_names)
        scene = capi.ExportedScene()
        if self.lib.export_scene(C.byref(scene), self._dev(), C.byref(source), int(bool(sort_triangles))):
            raise RuntimeError("export_scene failed")
        try:
            if path is not None and self.lib.write_exported_scene(C.byref(scene), str(path).encode()):
                raise RuntimeError("write_exported_scene failed for %s" % path)
            return scene_export.exported_buffers(scene)
        finally:
            self.lib.free_exported_scene(C.byref(scene))

    def fit_ltc_table(self, resolution=None, fresnel_count=None, sample_count=None, max_iterations=None):
        """Replaces the LTC table by one fitted on the device (include/vkr_ltc_table.h fit_ltc_table); None: the default
        of the setting (32, 51, 32, 200).  The fits stay with the renderer for ltc_fits() and write_ltc_table().  Returns
        the milliseconds the call took (kernel, read-back, quantisation and upload).  Frames in flight are finished
        first: they read the old table."""
        import time
        if self.app.shading_pass.constants_device:
            self.finish_frames()
            self.sync()
        settings = self.lib.get_default_ltc_fit_settings()
        for name, value in (("resolution", resolution), ("fresnel_count", fresnel_count), ("sample_count", sample_count), ("max_iterations", max_iterations)):
            if value is not None:
                setattr(settings, name, int(value))
        self._free_ltc_fits()
        self.lib.destroy_ltc_table(C.byref(self.app.ltc_table), self._dev())
        fits = C.POINTER(C.c_float)()
        start = time.perf_counter()
        if self.lib.fit_ltc_table(C.byref(self.app.ltc_table), C.byref(fits), self._dev(), C.byref(settings)):
            raise RuntimeError("fit_ltc_table failed")
        # (the size goes with the pointer: the table of the application may be replaced behind this object's back)
        self._ltc_fits, self._ltc_fit_size = fits, (int(settings.resolution), int(settings.fresnel_count))
        return (time.perf_counter() - start) * 1.0e3

    def ltc_fits(self):
        """The fits of the last fit_ltc_table(): (fresnel_count, R, R, 5) float32, [i, y, x], the order of the files"""
        if not getattr(self, "_ltc_fits", None):
            raise RuntimeError("no fitted LTC table: call fit_ltc_table() first")
        resolution, fresnel_count = self._ltc_fit_size
        return np.ctypeslib.as_array(self._ltc_fits, (fresnel_count, resolution, resolution, 5)).copy()

    def write_ltc_table(self, directory):
        """Writes the fits of the last fit_ltc_table() as <directory>/fit<i>.dat, which load_ltc_table() reads"""
        if not getattr(self, "_ltc_fits", None):
            raise RuntimeError("no fitted LTC table: call fit_ltc_table() first")
        resolution, fresnel_count = self._ltc_fit_size
        if self.lib.write_ltc_table(self._ltc_fits, resolution, fresnel_count, directory.encode()):
            raise RuntimeError("write_ltc_table failed for %s" % directory)

    def upload_visibility(self, visibility):
        v = np.ascontiguousarray(visibility, np.uint32)
        if self.lib.upload_visibility(C.byref(self.app), v.ctypes.data):
            raise RuntimeError("upload_visibility failed")

    def render_visibility(self):
        if self.lib.render_visibility_pass(C.byref(self.app)):
            raise RuntimeError("render_visibility_pass failed")

    def render(self, out_pointer=None):
        if self.lib.render_shading_pass(C.byref(self.app), out_pointer):
            raise RuntimeError("render_shading_pass failed")

    def next_frame_stream(self):
        return int(self.lib.get_next_frame_stream(C.byref(self.app)) or 0)

    def render_encoded(self, out_pointer, rgb8_pointer):
        if self.lib.render_shading_pass_encoded(C.byref(self.app), out_pointer, rgb8_pointer):
            raise RuntimeError("render_shading_pass_encoded failed")

    def last_ms(self):
        return float(self.lib.get_last_dispatch_milliseconds(C.byref(self.app)))

    def dispatch_ms(self, count):
        out = (C.c_float * count)()
        n = self.lib.get_dispatch_milliseconds(C.byref(self.app), out, count)
        return [float(out[i]) for i in range(n)]

    def shading_kernel_ms(self, count):
        out = (C.c_float * count)()
        n = self.lib.get_shading_kernel_milliseconds(C.byref(self.app), out, count)
        return [float(out[i]) for i in range(n)]

    def light_shaft_ms(self, count):
        out = (C.c_float * count)()
        n = self.lib.get_light_shaft_milliseconds(C.byref(self.app), out, count)
        return [float(out[i]) for i in range(n)]

    def frame_period_ms(self, count):
        out = (C.c_float * count)()
        n = self.lib.get_frame_period_milliseconds(C.byref(self.app), out, count)
        return [float(out[i]) for i in range(n)]

    def finish_frames(self):
        if self.lib.finish_frames(C.byref(self.app)):
            raise RuntimeError("finish_frames failed")

    def last_ray_count(self):
        return int(self.lib.get_last_ray_count(C.byref(self.app)))

    def traversal_statistics(self, wide_tree=None):
        """Work of the BVH traversal for the rays of the last wavefront frame (diagnostics).
        wide_tree None: the tree the frame walked; True / False: the four-wide / the binary one."""
        out = (C.c_uint64 * 12)()
        if wide_tree is None:
            wide_tree = bool(self.app.scene.acceleration_structure.wide_nodes) and not self.app.shading_pass.binary_traversal
        if self.lib.get_traversal_statistics_of_tree(C.byref(self.app), int(wide_tree), out):
            raise RuntimeError("get_traversal_statistics_of_tree failed")
        keys = ("rays", "node_visits", "triangle_tests", "blocked_rays", "wave_steps", "longest_ray_visits", "boxes_tested", "deepest_stack", "rays_beyond_lds_stack", "node_visits_of_blocked_rays")
        stats = dict(zip(keys, (int(v) for v in out)))
        stats["tree"] = "wide" if wide_tree else "binary"
        if not wide_tree:
            stats["boxes_tested"] = stats["node_visits"]
            for key in ("deepest_stack", "rays_beyond_lds_stack", "node_visits_of_blocked_rays"):
                del stats[key]
        return stats

    def light_shaft_statistics(self):
        """(patch, light) pairs of the last launch and how many of them needed no shadow rays (csrc/light_shafts.h)"""
        out = (C.c_uint64 * 12)()
        if self.lib.get_light_shaft_statistics(C.byref(self.app), out):
            raise RuntimeError("get_light_shaft_statistics failed")
        work = (C.c_uint64 * 3)()
        self.lib.get_light_shaft_work(C.byref(self.app), work)
        return {"pairs": int(out[0]), "clear_pairs": int(out[1]), "patches": int(out[2]), "lights": int(out[3]), "work": {"steps": int(work[0]), "triangle_batches": int(work[1]), "walks": int(work[2])},
                "not_clear": {"no_shaded_pixel": int(out[4]), "no_shaft": int(out[5]), "walk_too_long": int(out[6]), "queue_full": int(out[7]), "triangle_in_the_way": int(out[8]), "other": int(out[9])},
                # pairs whose rays the shading kernel decides against a handful of triangles, and those triangles
                "list_pairs": int(out[10]), "listed_triangles": int(out[11])}

    def prepared_polygon_statistics(self):
        """How the last launch got its prepared polygons ("plain", "storing", "loading") and the state of the cache that
        keeps them while the inputs stand still (include/vkr_shading_pass.h get_prepared_polygon_statistics)"""
        out = (C.c_uint64 * 8)()
        self.lib.get_prepared_polygon_statistics(C.byref(self.app), out)
        return {"mode": ("plain", "storing", "loading")[int(out[0])], "buffer_bytes": int(out[1]),
                "launches": {"plain": int(out[2]), "storing": int(out[3]), "loading": int(out[4])}, "waited": int(out[5]),
                "state": ("empty", "pending", "valid")[int(out[6])], "budget_mib": int(out[7])}

    def sector_terms_statistics(self):
        """The sector terms that are kept with the prepared polygons where both fit: bytes of their buffer and the loading
        launches so far with and without terms (include/vkr_shading_pass.h get_sector_terms_statistics)"""
        out = (C.c_uint64 * 3)()
        self.lib.get_sector_terms_statistics(C.byref(self.app), out)
        return {"buffer_bytes": int(out[0]), "loaded_with_terms": int(out[1]), "loaded_without_terms": int(out[2])}

    def light_shaft_words(self):
        """The verdict words of the last launch as a (patches, lights) uint32 array (include/vkr_shading_pass.h
        read_back_light_shafts); empty when that launch ran without the shaft test"""
        lights = int(self.app.scene_specification.polygonal_light_count)
        words = np.zeros(int(self.app.shading_pass.last_shaft_groups) * lights, np.uint32)
        got = int(self.lib.read_back_light_shafts(C.byref(self.app), words.ctypes.data, words.size)) if words.size else 0
        return words[:got].reshape(-1, max(lights, 1))

    def mark_inputs_changed(self):
        """An input of the pass in device memory was rewritten by someone else: frames in flight wait for device->stream
        once, and no light shaft verdict of an earlier frame is kept"""
        self.lib.mark_inputs_changed(C.byref(self.app))

    # -- multi-GPU exchange (include/vkr_slab_exchange.h) ---------------------------------
    def exchange_id(self):
        """The rendezvous token of a new communicator as 128 bytes (call on one rank, broadcast)."""
        token = capi.SlabExchangeId()
        if self.lib.get_slab_exchange_id(C.byref(token)):
            raise RuntimeError("get_slab_exchange_id failed (RCCL missing?)")
        return bytes(C.string_at(C.byref(token), 128))

    def create_exchange(self, token_bytes, slab_format="rgba32f"):
        token = capi.SlabExchangeId()
        C.memmove(C.byref(token), token_bytes, 128)
        self.exchange = capi.SlabExchange()
        if self.lib.create_slab_exchange(C.byref(self.exchange), C.byref(self.app), C.byref(token), capi.SLAB_FORMAT[slab_format]):
            self.exchange = None
            raise RuntimeError("create_slab_exchange failed")

    def create_exchange_with_gather(self, gather, slab_format="rgba32f"):
        """An exchange whose collective is the Python callable gather(rank, set, send_pointer, gathered_pointer,
        send_bytes, stream) -> 0 on success (include/vkr_slab_exchange.h slab_gather_function_t): any transport
        the caller has, e.g. a host-staged all-gather over a CPU process group."""
        prototype = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p)

        def trampoline(context, rank, buffer_set, send, gathered, send_bytes, stream):
            try:
                return int(gather(int(rank), int(buffer_set), int(send or 0), int(gathered or 0), int(send_bytes), int(stream or 0)))
            except Exception as error:  # an exception must not unwind through the C frames
                print("slab gather callback failed: %r" % (error,), flush=True)
                return 1
        self._gather_keepalive = prototype(trampoline)
        self.exchange = capi.SlabExchange()
        if self.lib.create_slab_exchange_with_gather(C.byref(self.exchange), C.byref(self.app), C.cast(self._gather_keepalive, C.c_void_p), None, capi.SLAB_FORMAT[slab_format]):
            self.exchange = None
            raise RuntimeError("create_slab_exchange_with_gather failed")

    def create_local_exchange(self, group, slab_format="rgba32f"):
        """Joins a group made by capi.load().create_local_slab_group(rank_count): ranks of this process that
        exchange their slabs with device-to-device copies (call from the rank's own thread)"""
        self.exchange = capi.SlabExchange()
        if self.lib.create_local_slab_exchange(C.byref(self.exchange), C.byref(self.app), group, capi.SLAB_FORMAT[slab_format]):
            self.exchange = None
            raise RuntimeError("create_local_slab_exchange failed")

    def assemble_on_demand(self, on=True):
        """The frame stays tile-major - the gathered slabs - until a reader asks for it (finish_exchange(), assemble_exchanged());
        include/vkr_slab_exchange.h slab_exchange_t.assemble_on_demand"""
        self.exchange.assemble_on_demand = int(bool(on))

    def assemble_exchanged(self, out_pointer=None):
        if self.lib.assemble_exchanged_frame(C.byref(self.app), C.byref(self.exchange), out_pointer):
            raise RuntimeError("assemble_exchanged_frame failed")

    def destroy_exchange(self):
        if self.exchange is not None:
            self.lib.destroy_slab_exchange(C.byref(self.exchange), C.byref(self.app))
            self.exchange = None

    def render_and_exchange(self, out_pointer=None):
        if self.lib.render_and_exchange_frame(C.byref(self.app), C.byref(self.exchange), out_pointer):
            raise RuntimeError("render_and_exchange_frame failed")

    def finish_exchange(self):
        if self.lib.finish_slab_exchange(C.byref(self.app), C.byref(self.exchange)):
            raise RuntimeError("finish_slab_exchange failed")

    def exchange_ms(self):
        """(shade, all-gather, scatter) of the most recent timed frame, or None"""
        out = (C.c_float * 3)()
        if not self.lib.get_slab_exchange_milliseconds(C.byref(self.exchange), out):
            return None
        return [float(v) for v in out]

    def sync(self):
        self.lib.wait_for_device(C.byref(self.app.device))

    def read_radiance(self):
        e = self.app.swapchain.extent
        out = np.zeros((e.height, e.width, 4), np.float32)
        if self.lib.read_back_radiance(C.byref(self.app), out.ctypes.data):
            raise RuntimeError("read_back_radiance failed")
        return out

    def begin_read_back(self, slot=0, pointer=None, nbytes=0):
        """Queues the copy of a device buffer (default: the radiance target) into the slot's pinned staging memory behind
        the most recent frame and returns at once (include/vkr_shading_pass.h begin_read_back)"""
        if self.lib.begin_read_back(C.byref(self.app), slot, pointer, nbytes):
            raise RuntimeError("begin_read_back failed")

    def end_read_back(self, slot=0, shape=None, dtype=np.float32):
        """Waits for the slot's copy; returns a numpy VIEW of the pinned staging memory (valid until the slot's next
        begin_read_back), shaped like the radiance target unless `shape` says otherwise"""
        address = self.lib.end_read_back(C.byref(self.app), slot)
        if not address:
            raise RuntimeError("end_read_back failed")
        if shape is None:
            e = self.app.swapchain.extent
            shape = (e.height, e.width, 4)
        count = int(np.prod(shape))
        buffer = (C.c_char * (count * np.dtype(dtype).itemsize)).from_address(address)
        return np.frombuffer(buffer, dtype=dtype, count=count).reshape(shape)

    def read_visibility(self):
        e = self.app.swapchain.extent
        out = np.zeros((e.height, e.width), np.uint32)
        if self.lib.read_back_visibility(C.byref(self.app), out.ctypes.data):
            raise RuntimeError("read_back_visibility failed")
        return out

    # -- feature buffers (include/vkr_feature_buffers.h) -----------------------------------
    def render_features(self, names, reprojection_matrix=None, pointers=None):
        """The feature images of the current frame (render_feature_buffers): names out of capi.PIXEL_FEATURES;
        reprojection_matrix: a (4, 4) world_to_projection_space for "reprojection" (default: this frame's own).
        -> {name: array (height, width, 4)}, float32 or, for "identity", uint32.  With pointers, {name: device address}
        for every name, the images stay on the device, the call returns once the kernel is queued and gives nothing."""
        from . import feature_buffers
        names = [names] if isinstance(names, str) else list(names)
        buffers = capi.FeatureBuffers()
        if reprojection_matrix is None:
            reprojection_matrix = feature_buffers.world_to_projection_space(self.constants())
        matrix = np.ascontiguousarray(reprojection_matrix, np.float32).reshape(4, 4)
        for i in range(4):
            buffers.reprojection_matrix[i][:] = [float(v) for v in matrix[i]]
        e = self.app.swapchain.extent
        nbytes = e.width * e.height * 16
        with _DeviceScratch(self, "the feature images") as scratch:
            for name in names:
                index = capi.PIXEL_FEATURES.index(name)
                buffers.images[index] = int(pointers[name]) if pointers is not None else scratch.allocate(nbytes, "the %s image" % name)
            if self.lib.render_feature_buffers(C.byref(self.app), C.byref(buffers)):
                raise RuntimeError("render_feature_buffers failed")
            if pointers is not None:
                return None
            self.sync()
            return {name: scratch.download(buffers.images[capi.PIXEL_FEATURES.index(name)], (e.height, e.width, 4), np.uint32 if name == "identity" else np.float32, "the %s image" % name)
                    for name in names}

    # -- motion buffers (include/vkr_motion_buffers.h) --------------------------------------
    def render_motion(self, previous_positions, previous_matrix, names=capi.MOTION_IMAGES, pointers=None):
        """The motion images of the current frame (render_motion_buffers): names out of capi.MOTION_IMAGES.
        previous_positions: the position words of the mesh before the last update_geometry(), an array as that call takes
        it - (3 T, 2) uint32, which is uploaded - or a device address; None: nothing moved.  previous_matrix: the (4, 4)
        world_to_projection_space of the previous frame.  -> {name: float32 array (height, width, 4)}.  With pointers,
        {name: device address} for every name, the images stay on the device, the call returns once the kernel is queued
        and gives nothing (previous_positions as an array is then waited for: it is freed on the way out)."""
        names = [names] if isinstance(names, str) else list(names)
        buffers = capi.MotionBuffers()
        matrix = np.ascontiguousarray(previous_matrix, np.float32).reshape(4, 4)
        for i in range(4):
            buffers.previous_matrix[i][:] = [float(v) for v in matrix[i]]
        e = self.app.swapchain.extent
        nbytes = e.width * e.height * 16
        with _DeviceScratch(self, "the motion images") as scratch:
            if isinstance(previous_positions, np.ndarray):
                words = np.ascontiguousarray(previous_positions, np.uint32)
                vertex_count = 3 * int(self.app.scene.mesh.triangle_count)
                if words.size != 2 * vertex_count:
                    raise ValueError("expected %d x 2 uint32 for the %d triangles of the mesh, got %d values" % (vertex_count, vertex_count // 3, words.size))
                buffers.previous_positions = scratch.upload(words, dtype=None, what="the previous positions")
            elif previous_positions is not None:
                buffers.previous_positions = _address(previous_positions)
            for name in names:
                if name not in capi.MOTION_IMAGES:
                    raise ValueError("%r is no motion image (%s)" % (name, ", ".join(capi.MOTION_IMAGES)))
                setattr(buffers, name, int(pointers[name]) if pointers is not None else scratch.allocate(nbytes, "the %s image" % name))
            if self.lib.render_motion_buffers(C.byref(self.app), C.byref(buffers)):
                raise RuntimeError("render_motion_buffers failed")
            if pointers is not None:
                return None
            self.sync()
            return {name: scratch.download(getattr(buffers, name), (e.height, e.width, 4), np.float32, "the %s image" % name) for name in names}

    def feature_preview(self, name, image_or_pointer, range=(0.0, 1.0), out_pointer=None):
        """The RGBA8 preview of a feature image (encode_feature_preview) - an array as render_features() returns it, which
        is uploaded, or a device address.  range: (low, high) for "position" (distances) and "reprojection" (high: the
        motion in pixels that saturates).  -> uint8 array (height, width, 4); with out_pointer, a device address, the
        preview stays there (for encode_png() / encode_jpeg()) and the call returns once the kernel is queued."""
        e = self.app.swapchain.extent
        with _DeviceScratch(self, "the preview") as scratch:
            source = image_or_pointer
            if isinstance(image_or_pointer, np.ndarray):
                if image_or_pointer.shape != (e.height, e.width, 4) or image_or_pointer.dtype.itemsize != 4:
                    raise ValueError("a feature image is (height, width, 4) of 32-bit values")
                source = scratch.upload(image_or_pointer, dtype=None, what="the feature image")
            target = out_pointer if out_pointer is not None else scratch.allocate(e.width * e.height * 4)
            feature = capi.PIXEL_FEATURES.index(name) if isinstance(name, str) else int(name)
            if self.lib.encode_feature_preview(C.byref(self.app), feature, source, target, float(range[0]), float(range[1])):
                raise RuntimeError("encode_feature_preview failed")
            if out_pointer is not None:
                return None
            self.sync()
            return scratch.download(target, (e.height, e.width, 4), np.uint8, "the preview")

    # -- ray queries (include/vkr_ray_queries.h) ------------------------------------------
    def _trace(self, closest, origins, directions, t_min, t_max, cull_back_faces, walk, lds_stack_entries, rays_pointer, out_pointer, count, stream):
        """Both ray queries.  Host arrays are uploaded and the answers read back (a blocking call); with rays_pointer and
        out_pointer - device memory of `count` records - nothing is copied and the call returns once it is enqueued."""
        from . import ray_queries
        hip = C.CDLL("libamdhip64.so")
        # (an int, a ctypes pointer or None: the address, None for the device's stream)
        stream = C.cast(stream, C.c_void_p).value if isinstance(stream, (C._SimpleCData, C._Pointer)) else (int(stream) if stream else None)
        waited_for = C.c_void_p(stream or self.app.device.stream)
        options = capi.RayQueryOptions(_enum(ray_queries.WALK, walk), int(lds_stack_entries))
        record = ray_queries.HIT if closest else np.dtype(np.uint8)
        owned = []

        def allocate(nbytes):
            pointer = C.c_void_p()
            if hip.hipMalloc(C.byref(pointer), C.c_size_t(max(nbytes, 1))):
                raise RuntimeError("out of device memory for %d bytes of a ray query" % nbytes)
            owned.append(pointer)
            return pointer

        try:
            if rays_pointer is None:
                rays = ray_queries.make_rays(origins, directions, t_min, t_max)
                count = len(rays)
                rays_pointer = allocate(rays.nbytes)
                if count and hip.hipMemcpy(rays_pointer, C.c_void_p(rays.ctypes.data), C.c_size_t(rays.nbytes), 1):
                    raise RuntimeError("uploading the rays failed")
            elif count is None:
                raise ValueError("rays_pointer needs count")
            read_back = out_pointer is None
            if read_back:
                out_pointer = allocate(record.itemsize * count)
            scene, device = C.byref(self.app.scene), self._dev()
            if closest:
                failed = self.lib.trace_closest_hits(scene, device, rays_pointer, count, int(bool(cull_back_faces)), out_pointer, C.byref(options), stream)
            else:
                failed = self.lib.trace_any_hits(scene, device, rays_pointer, count, out_pointer, C.byref(options), stream)
            if failed:
                raise RuntimeError("%s failed" % ("trace_closest_hits" if closest else "trace_any_hits"))
            if not read_back:
                return None
            out = np.zeros(count, record)
            # (hipMemcpy does not wait for a non-blocking stream)
            if hip.hipStreamSynchronize(waited_for) or (count and hip.hipMemcpy(C.c_void_p(out.ctypes.data), out_pointer, C.c_size_t(out.nbytes), 2)):
                raise RuntimeError("reading the answers of the ray query back failed")
            return out if closest else out.astype(bool)
        finally:
            if owned:
                hip.hipStreamSynchronize(waited_for)
            for pointer in owned:
                hip.hipFree(pointer)

    def trace_closest_hits(self, origins=None, directions=None, t_min=1.0e-3, t_max=np.inf, cull_back_faces=False, walk="auto", rays_pointer=None, hits_pointer=None, count=None, lds_stack_entries=0, stream=None):
        """The closest hit of every ray o + t d, t in [t_min, t_max], with the triangles of the loaded scene
        (include/vkr_ray_queries.h trace_closest_hits): a structured array of ray_queries.HIT - primitive (0xFFFFFFFF:
        none), t, u, v.  origins, directions: (n, 3); t_min, t_max: scalars or (n,).  rays_pointer, hits_pointer: device
        memory of `count` ray_t / ray_hit_t instead of the arrays / the return value; stream: a hipStream_t instead of
        the device's."""
        return self._trace(True, origins, directions, t_min, t_max, cull_back_faces, walk, lds_stack_entries, rays_pointer, hits_pointer, count, stream)

    def trace_any_hits(self, origins=None, directions=None, t_min=1.0e-3, t_max=np.inf, walk="auto", rays_pointer=None, blocked_pointer=None, count=None, lds_stack_entries=0, stream=None):
        """Whether anything blocks the segments t in [t_min, t_max] of the rays (trace_any_hits): a bool array; the
        arguments of trace_closest_hits(), blocked_pointer one byte per ray"""
        return self._trace(False, origins, directions, t_min, t_max, False, walk, lds_stack_entries, rays_pointer, blocked_pointer, count, stream)

    def pixel_rays(self):
        """The pixel-centre rays of the current camera and extent, raster order, as ray_queries.RAY records: what
        render_visibility_pass() traces, built from the same bytes of the constant buffer"""
        from . import ray_queries
        e, camera = self.app.swapchain.extent, self.app.scene_specification.camera
        return ray_queries.pixel_rays(self.constants(), e.width, e.height, camera.near, camera.far)

    def pick(self, x, y):
        """The front-facing triangle under the centre of pixel (x, y): one ray_queries.HIT record"""
        e = self.app.swapchain.extent
        if not (0 <= x < e.width and 0 <= y < e.height):
            raise ValueError("pixel (%d, %d) is outside the %d x %d frame" % (x, y, e.width, e.height))
        ray = self.pixel_rays()[y * e.width + x:y * e.width + x + 1]
        return self.trace_closest_hits(ray["origin"], ray["direction"], ray["t_min"], ray["t_max"], cull_back_faces=True)[0]

    # -- moving geometry (include/vkr_scene_update.h) -------------------------------------
    def update_geometry(self, positions, normals_and_tex_coords=None, policy="refit", on_device=False, measure_cost=False, rebuild_above=0.0, refresh_host_copy=True):
        """New vertex positions for the loaded mesh (update_scene_geometry): the file's words, (3 T, 2) uint32 - see
        scene_update.pack_positions() - or, with on_device, the address of such an array in device memory; likewise
        normals_and_tex_coords, (3 T, 4) uint16, or None to keep them.  policy: "refit", "rebuild" or "auto" (rebuild when
        the refitted tree costs more than rebuild_above times the tree as built).  Waits for the frames in flight first.
        -> the report as a dict; call render_visibility() before the next render()."""
        from . import scene_update
        self.finish_frames()
        vertex_count = 3 * int(self.app.scene.mesh.triangle_count)
        keep = []

        def pointer(array, dtype, width):
            if array is None:
                return None
            if on_device:
                return C.cast(array, C.c_void_p).value if isinstance(array, (C._SimpleCData, C._Pointer)) else int(array)
            array = np.ascontiguousarray(array, dtype)
            if array.size != vertex_count * width:
                raise ValueError("expected %d x %d %s for the %d triangles of the mesh, got %d values" % (vertex_count, width, np.dtype(dtype).name, vertex_count // 3, array.size))
            keep.append(array)
            return array.ctypes.data
        options = capi.SceneUpdateOptions(_enum(scene_update.POLICY, policy), int(bool(on_device)), int(bool(refresh_host_copy)), int(bool(measure_cost)), float(rebuild_above))
        report = capi.SceneUpdateReport()
        if self.lib.update_scene_geometry(C.byref(self.app.scene), self._dev(), pointer(positions, np.uint32, 2), pointer(normals_and_tex_coords, np.uint16, 4), C.byref(options), C.byref(report)):
            raise RuntimeError("update_scene_geometry failed")
        return {"rebuilt": bool(report.rebuilt), "build_serial": int(report.build_serial), "milliseconds": float(report.milliseconds),
                "cost": float(report.cost), "built_cost": float(report.built_cost)}

    def read_acceleration_structure(self):
        """The acceleration structure as numpy arrays, read back from the device: nodes (N, 4) uint32 and wide_nodes
        (W, 16) uint32 (csrc/lbvh.h; None without a wide tree), triangle_vertices (3 L, 4) float32, leaf_fragments (L,)
        uint32 (slab j << 16 | count per leaf slot), grid_origin and grid_inverse_cell (3,) float32, and the counts, the
        builder and build_serial as ints"""
        s = self.app.scene.acceleration_structure
        if not s.nodes:
            raise RuntimeError("the scene has no acceleration structure")
        hip = _hip_runtime()
        self.finish_frames()
        self.sync()

        def read(address, shape, dtype):
            out = np.zeros(shape, dtype)
            if out.nbytes and hip.hipMemcpy(out.ctypes.data, address, out.nbytes, 2):
                raise RuntimeError("reading the acceleration structure back failed")
            return out
        tree = {k: int(getattr(s, k)) for k in ("node_count", "leaf_count", "wide_node_count", "wide_stack_need", "builder", "build_serial")}
        tree["nodes"] = read(s.nodes, (s.node_count, 4), np.uint32)
        tree["wide_nodes"] = read(s.wide_nodes, (s.wide_node_count, 16), np.uint32) if s.wide_nodes else None
        tree["triangle_vertices"] = read(s.triangle_vertices, (3 * s.leaf_count, 4), np.float32)
        tree["leaf_fragments"] = read(s.leaf_fragments, (s.leaf_count,), np.uint32)
        tree["grid_origin"], tree["grid_inverse_cell"] = np.array(s.grid_origin[:], np.float32), np.array(s.grid_inverse_cell[:], np.float32)
        return tree

    def read_encoded(self, output_linear_rgb=False, frame_bits=0):
        e = self.app.swapchain.extent
        self.app.screenshot.frame_bits = frame_bits
        if self.lib.encode_output(C.byref(self.app), int(output_linear_rgb)):
            raise RuntimeError("encode_output failed")
        out = np.zeros((e.height, e.width, 4), np.uint8)
        if self.lib.read_back_encoded(C.byref(self.app), out.ctypes.data):
            raise RuntimeError("read_back_encoded failed")
        self.app.screenshot.frame_bits = 0
        return out

    # -- JPEG, Radiance and PNG files (include/vkr_jpeg.h, vkr_hdr.h, vkr_png.h) ------------------
    def _create_file_encoder(self, encoder_class, width, height, *arguments):
        """An open encoder of that class for one extent (default: the frame's); `arguments`: what its constructor takes
        behind the extent"""
        e = self.app.swapchain.extent
        encoder = encoder_class(self, int(width or e.width), int(height or e.height), *arguments)
        self._file_encoders.append(encoder)
        return encoder

    def _cached_file_encoder(self, encoder_class, *key):
        """The one-slot encoder of that class that is kept per `key`: the extent, for JPEG also the quality"""
        key = (encoder_class,) + tuple(int(k) for k in key)
        cache = self._file_encoder_cache
        if key not in cache or cache[key].closed:
            cache[key] = self._create_file_encoder(*key)
        return cache[key]

    def _encode_file(self, encoder_class, image_or_pointer, width, height, channel_count, row_stride_bytes, key=(), format_arguments=()):
        """The file of a numpy image, which is uploaded, or of device memory at an address; key: what the cached encoder is
        kept by besides the extent; format_arguments: what the format's C functions take besides the pixels"""
        if isinstance(image_or_pointer, np.ndarray):
            image = np.ascontiguousarray(image_or_pointer, encoder_class.DTYPE)
            if image.ndim != 3 or image.shape[2] not in (3, 4):
                raise ValueError("%s files are made from %s images of shape (height, width, 3 or 4)" % (encoder_class.FORMAT.upper(), encoder_class.DTYPE.__name__))
            return self._cached_file_encoder(encoder_class, image.shape[1], image.shape[0], *key)._encode_image(image, 0, *format_arguments)
        e = self.app.swapchain.extent
        encoder = self._cached_file_encoder(encoder_class, width or e.width, height or e.height, *key)
        encoder._begin(0, image_or_pointer, channel_count, row_stride_bytes, None, *format_arguments)
        return encoder.end(0)

    def create_jpeg_encoder(self, width=None, height=None, quality=70, slot_count=1):
        """An encoder for frames of one extent (default: the frame's) and quality with `slot_count` output slots: a
        JpegEncoder, which exposes begin() and end() per slot.  The caller closes it (Renderer.close() closes what is left)."""
        return self._create_file_encoder(JpegEncoder, width, height, quality, slot_count)

    def encode_jpeg(self, image_or_pointer, quality=70, width=None, height=None, channel_count=4, row_stride_bytes=0):
        """The bytes of the JPEG file of an image - a uint8 array (height, width, 3 or 4), which is uploaded - or of
        device memory (an address; width, height default to the frame's extent; channel_count 3 or 4, rows
        row_stride_bytes apart).  Byte for byte what jpeg.encode() gives.  The encoder is kept for the next call with
        the same extent and quality."""
        return self._encode_file(JpegEncoder, image_or_pointer, width, height, channel_count, row_stride_bytes, key=(quality,))

    def read_jpeg(self, quality=70):
        """The current frame as a JPEG file: the sRGB-encoded frame of read_encoded(), encoded on the device, so that
        only the file crosses the bus"""
        self.app.screenshot.frame_bits = 0
        if self.lib.encode_output(C.byref(self.app), 0):
            raise RuntimeError("encode_output failed")
        return self.encode_jpeg(self.app.render_targets.encoded, quality)

    def create_hdr_encoder(self, width=None, height=None, slot_count=1):
        """An encoder for float frames of one extent (default: the frame's) with `slot_count` output slots: an HdrEncoder,
        which exposes begin() and end() per slot.  The caller closes it (Renderer.close() closes what is left)."""
        return self._create_file_encoder(HdrEncoder, width, height, slot_count)

    def encode_hdr(self, image_or_pointer, through_half=False, width=None, height=None, channel_count=4, row_stride_bytes=0):
        """The bytes of the Radiance file of an image - a float32 array (height, width, 3 or 4), which is uploaded - or of
        device memory (an address; width, height default to the frame's extent; channel_count 3 or 4 floats, rows
        row_stride_bytes apart).  Byte for byte what hdr.encode() gives.  The encoder is kept for the next call with
        the same extent."""
        return self._encode_file(HdrEncoder, image_or_pointer, width, height, channel_count, row_stride_bytes, format_arguments=(int(bool(through_half)),))

    def read_hdr(self, through_half=False):
        """The current radiance target as a Radiance file, encoded on the device, so that only the file crosses the bus;
        through_half: every channel through half precision first, as the screenshots of the reference"""
        if self.lib.finish_frames(C.byref(self.app)):
            raise RuntimeError("finish_frames failed")
        return self.encode_hdr(self.app.render_targets.radiance, through_half)

    def create_png_encoder(self, width=None, height=None, slot_count=1):
        """An encoder for 8-bit frames of one extent (default: the frame's) with `slot_count` output slots: a PngEncoder,
        which exposes begin() and end() per slot.  The caller closes it (Renderer.close() closes what is left)."""
        return self._create_file_encoder(PngEncoder, width, height, slot_count)

    def encode_png(self, image_or_pointer, width=None, height=None, channel_count=4, row_stride_bytes=0):
        """The bytes of the PNG file of an image - a uint8 array (height, width, 3 or 4), which is uploaded - or of device
        memory (an address; width, height default to the frame's extent; channel_count 3 or 4 bytes, rows
        row_stride_bytes apart).  Byte for byte what png.encode() gives.  The encoder is kept for the next call with the
        same extent."""
        return self._encode_file(PngEncoder, image_or_pointer, width, height, channel_count, row_stride_bytes)

    def read_png(self, output_linear_rgb=False):
        """The current frame as a PNG file of its sRGB8 encoding (the RGB of read_encoded()), encoded on the device, so that
        only the file crosses the bus"""
        before = self.app.screenshot.frame_bits
        self.app.screenshot.frame_bits = 0
        try:
            if self.lib.encode_output(C.byref(self.app), int(output_linear_rgb)):
                raise RuntimeError("encode_output failed")
        finally:
            self.app.screenshot.frame_bits = before
        return self.encode_png(self.app.render_targets.encoded)

    def probe_png_stream(self, stream):
        """probe_png_stream() of include/vkr_png.h: the file the device makes of a filtered stream of the caller's, a uint8
        array (rows, row_length)"""
        stream = np.ascontiguousarray(stream, np.uint8)
        rows, row_length = stream.shape
        capacity = int(self.lib.get_png_stream_capacity(row_length, rows))
        out, size = np.zeros(capacity, np.uint8), C.c_uint64()
        if capacity == 0 or self.lib.probe_png_stream(self._dev(), C.c_void_p(stream.ctypes.data), row_length, rows, C.c_void_p(out.ctypes.data), capacity, C.byref(size)):
            raise RuntimeError("probe_png_stream failed")
        if size.value > capacity:
            raise RuntimeError("a file of %d bytes exceeds the capacity of %d" % (size.value, capacity))
        return out[:size.value].tobytes()

    def slab_pixel_count(self, rank=0):
        return int(self.lib.get_slab_pixel_count(C.byref(self.app), rank))

    def encode_slab(self, slab_pointer, encoded_pointer, pixel_count, output_linear_rgb=False):
        if self.lib.encode_slab(C.byref(self.app), slab_pointer, encoded_pointer, pixel_count, int(output_linear_rgb)):
            raise RuntimeError("encode_slab failed")

    def encode_slab_rgb8(self, slab_pointer, packed_pointer, pixel_count, output_linear_rgb=False):
        if self.lib.encode_slab_rgb8(C.byref(self.app), slab_pointer, packed_pointer, pixel_count, int(output_linear_rgb)):
            raise RuntimeError("encode_slab_rgb8 failed")

    def assemble_rgb8(self, gathered_pointer, out_pointer=None):
        if self.lib.assemble_rgb8_frame_from_slabs(C.byref(self.app), gathered_pointer, out_pointer):
            raise RuntimeError("assemble_rgb8_frame_from_slabs failed")

    def assemble_encoded(self, gathered_pointer, out_pointer=None):
        if self.lib.assemble_encoded_frame_from_slabs(C.byref(self.app), gathered_pointer, out_pointer):
            raise RuntimeError("assemble_encoded_frame_from_slabs failed")

    def assemble(self, gathered_pointer, out_pointer=None):
        if self.lib.assemble_frame_from_slabs(C.byref(self.app), gathered_pointer, out_pointer):
            raise RuntimeError("assemble_frame_from_slabs failed")

    # -- frame statistics (include/vkr_frame_statistics.h) ---------------------------------
    def create_statistics(self, pixel_count=None):
        """Per-pixel sums of frames on the device; pixel_count None: the frame of the swapchain extent"""
        return FrameStatistics(self, pixel_count)

    def squared_error(self, a, b, pixel_count):
        """Sum over pixels of (a - b)^2 per R, G, B for two RGBA32F device buffers, as three doubles"""
        out = (C.c_double * 3)()
        if self.lib.sum_squared_differences(C.byref(self.app), a, b, pixel_count, out):
            raise RuntimeError("sum_squared_differences failed")
        return np.array(out[:], np.float64)

    def frame_sum(self, a, pixel_count):
        """Sum over pixels per R, G, B of an RGBA32F device buffer, as three doubles"""
        out = (C.c_double * 3)()
        if self.lib.sum_frame(C.byref(self.app), a, pixel_count, out):
            raise RuntimeError("sum_frame failed")
        return np.array(out[:], np.float64)

    # -- frame filter (include/vkr_frame_filter.h) -----------------------------------------
    def create_frame_filter(self, width=None, height=None):
        """The scratch images of filter_frame() for frames of an extent; None: the swapchain extent"""
        return FrameFilter(self, width, height)

    def filter_frame(self, colour, variance, features, settings=None, modulation=None, out_colour=None, out_variance=None, frame_filter=None):
        """The edge-avoiding a-trous filter of include/vkr_frame_filter.h.  colour, variance (None: no luminance weight) and
        the values of features - {"position", "normal"} and, unless `modulation` names another image, optionally
        "diffuse_albedo", which colour is divided by before and multiplied by after - are device addresses or float32
        arrays (height, width, 4), which are uploaded.  settings: the members of frame_filter_settings_t that differ from
        frame_filter.DEFAULT_SETTINGS.  frame_filter: a create_frame_filter() of the images' extent; None: one of the
        swapchain extent that the renderer keeps.  -> (filtered colour, filtered variance or None) as arrays; with
        out_colour (and out_variance), device addresses, the results stay there, the call returns once the kernels are
        queued and gives nothing."""
        if frame_filter is None:
            frame_filter = self._kept_for_the_frame(FrameFilter)
        if modulation is None:
            modulation = features.get("diffuse_albedo")
        return frame_filter.apply(colour, variance, features["position"], features["normal"], modulation, settings, out_colour, out_variance)

    # -- frame history (include/vkr_frame_history.h) ---------------------------------------
    def create_frame_history(self, width=None, height=None):
        """A reprojected history of accumulate_frame_history() for frames of an extent; None: the swapchain extent"""
        return FrameHistory(self, width, height)

    def accumulate_history(self, colour, features, settings=None, modulation=None, out_colour=None, out_variance=None, want_variance=True, frame_history=None):
        """The temporal accumulation of include/vkr_frame_history.h.  colour and the values of features - {"position",
        "normal"}, optionally "reprojection" (under the previous frame's matrix; without it every pixel stays where it is),
        optionally "previous_position" (of render_motion(), with its reprojection: accumulate_moving_frame_history())
        and, unless `modulation` names another image, optionally "diffuse_albedo" - are device addresses or float32 arrays
        (height, width, 4), which are uploaded.  settings: the members of frame_history_settings_t that differ from
        frame_history.DEFAULT_SETTINGS.  frame_history: a create_frame_history() of the images' extent; None: one of the
        swapchain extent that the renderer keeps from call to call.  -> (accumulated colour, its variance or None without
        want_variance) as arrays; with out_colour (and out_variance), device addresses, the results stay there, the call
        returns once the kernels are queued and gives nothing."""
        if frame_history is None:
            frame_history = self._kept_for_the_frame(FrameHistory)
        return frame_history.accumulate(colour, features, settings, modulation, out_colour, out_variance, want_variance)

    def _kept_for_the_frame(self, frame_object_class):
        """The object of that class that the renderer keeps for the swapchain extent: made again when the extent changed
        or somebody closed it"""
        e = self.app.swapchain.extent
        kept = self._kept_frame_objects.get(frame_object_class)
        if kept is None or not kept.alive or (kept.width, kept.height) != (e.width, e.height):
            if kept is not None:
                kept.close()
            kept = self._kept_frame_objects[frame_object_class] = frame_object_class(self)
        return kept

    def close(self):
        for frame_object in list(self._frame_objects):
            frame_object.close()
        for encoder in self._file_encoders:
            encoder.close()
        super().close()


class _FileEncoder:
    """What JpegEncoder, HdrEncoder and PngEncoder are: create_<format>_encoder() of include/vkr_<format>.h for a
    Renderer.  encode() for one frame at a time, begin() and end() per slot for frames in flight, encode_on_device() for a
    file that stays in device memory.  `format_arguments` are what the format's C functions take besides the pixels."""
    # the format's name in the C function names, its struct of capi and the type of an image's channels
    FORMAT = STRUCT = DTYPE = None
    # what create_<format>_encoder() takes between the extent and the slot count
    create_arguments = ()

    def __init__(self, owner, width, height, slot_count=1):
        self.owner, self.lib = owner, owner.lib
        self.encoder = self.STRUCT()
        self.closed = True
        self._call("create_%s_encoder", owner._dev(), width, height, *self.create_arguments, slot_count)
        self.closed = False

    def _call(self, name, *arguments):
        name = name % self.FORMAT
        if getattr(self.lib, name)(C.byref(self.encoder), *arguments):
            raise RuntimeError(name + " failed")

    @property
    def capacity(self):
        return int(self.encoder.capacity)

    def _begin(self, slot, pointer, channel_count, row_stride_bytes, stream, *format_arguments):
        self._call("begin_%s_encode", slot, pointer, channel_count, row_stride_bytes, *format_arguments, stream)

    def begin(self, slot, pointer, channel_count=4, row_stride_bytes=0, stream=None):
        """Enqueues the encode of device memory on `stream` (None: the device's) into the slot and returns at once"""
        self._begin(slot, pointer, channel_count, row_stride_bytes, stream)

    def end(self, slot, copy=True):
        """Waits for the slot: the bytes of the file (copy=False: a numpy VIEW of the pinned staging memory, valid until
        the slot's next begin())"""
        address, size = C.c_void_p(), C.c_uint64()
        self._call("end_%s_encode", slot, C.byref(address), C.byref(size))
        if copy:
            return C.string_at(address.value, size.value)
        return np.frombuffer((C.c_uint8 * size.value).from_address(address.value), np.uint8)

    def encode(self, pointer, channel_count=4, row_stride_bytes=0):
        self._begin(0, pointer, channel_count, row_stride_bytes, None)
        return self.end(0)

    def _encode_image(self, image, row_stride_bytes, *format_arguments):
        image = np.ascontiguousarray(image, self.DTYPE)
        if image.shape[0] != self.encoder.height or image.shape[1] != self.encoder.width:
            raise ValueError("this encoder is for %d x %d images" % (self.encoder.width, self.encoder.height))
        row = image.shape[1] * image.shape[2] * image.itemsize
        stride = int(row_stride_bytes) or row
        # (a value in the padding between rows that would show if it were read)
        padded = np.full((image.shape[0], stride), 0xA5, np.uint8)
        padded[:, :row] = image.view(np.uint8).reshape(image.shape[0], row)
        hip = _hip_runtime()
        pointer = C.c_void_p()
        if hip.hipMalloc(C.byref(pointer), padded.nbytes):
            raise RuntimeError("out of device memory for an image of %d bytes" % padded.nbytes)
        try:
            if hip.hipMemcpy(pointer, padded.ctypes.data, padded.nbytes, 1):
                raise RuntimeError("uploading the image failed")
            self._begin(0, pointer, image.shape[2], stride, None, *format_arguments)
            return self.end(0)
        finally:
            hip.hipFree(pointer)

    def encode_image(self, image, row_stride_bytes=0):
        """Uploads an image (height, width, 3 or 4) of the format's type, rows row_stride_bytes apart on the device, and
        encodes it"""
        return self._encode_image(image, row_stride_bytes)

    def _encode_on_device(self, pointer, out_pointer, capacity, size_pointer, channel_count, row_stride_bytes, stream, *format_arguments):
        self._call("encode_%s_on_device", pointer, channel_count, row_stride_bytes, *format_arguments, out_pointer, capacity, size_pointer, stream)

    def encode_on_device(self, pointer, out_pointer, capacity, size_pointer, channel_count=4, row_stride_bytes=0, stream=None):
        """encode_<format>_on_device(): at most `capacity` bytes of the file to out_pointer, its size to the 8 bytes at
        size_pointer, both device memory; returns once it is enqueued"""
        self._encode_on_device(pointer, out_pointer, capacity, size_pointer, channel_count, row_stride_bytes, stream)

    def close(self):
        if not self.closed:
            self._call("destroy_%s_encoder")
            self.closed = True


class JpegEncoder(_FileEncoder):
    """uint8 images as JPEG files of one quality"""
    FORMAT, STRUCT, DTYPE = "jpeg", capi.JpegEncoder, np.uint8

    def __init__(self, owner, width, height, quality=70, slot_count=1):
        self.create_arguments = (int(quality),)
        super().__init__(owner, width, height, slot_count)


class PngEncoder(_FileEncoder):
    """uint8 images as PNG files"""
    FORMAT, STRUCT, DTYPE = "png", capi.PngEncoder, np.uint8


class HdrEncoder(_FileEncoder):
    """float32 images as Radiance files; through_half: every channel through half precision first"""
    FORMAT, STRUCT, DTYPE = "hdr", capi.HdrEncoder, np.float32

    def begin(self, slot, pointer, channel_count=4, row_stride_bytes=0, through_half=False, stream=None):
        self._begin(slot, pointer, channel_count, row_stride_bytes, stream, int(bool(through_half)))

    def encode(self, pointer, channel_count=4, row_stride_bytes=0, through_half=False):
        self.begin(0, pointer, channel_count, row_stride_bytes, through_half)
        return self.end(0)

    def encode_image(self, image, row_stride_bytes=0, through_half=False):
        return self._encode_image(image, row_stride_bytes, int(bool(through_half)))

    def encode_on_device(self, pointer, out_pointer, capacity, size_pointer, channel_count=4, row_stride_bytes=0, through_half=False, stream=None):
        self._encode_on_device(pointer, out_pointer, capacity, size_pointer, channel_count, row_stride_bytes, stream, int(bool(through_half)))


def frames_in_flight_for(rank_count):
    """Depth of the frame pipeline that bench.py and profiles/tools/predict_scaling.py use when the frame is tiled over
    `rank_count` GPUs.  Three frames like the reference's frame queue (main.c:1498); four when a rank's slab is an eighth
    of the frame or less: its kernels then last about as long as their slowest wave, whatever the slab's size, and one more
    frame in flight fills what that leaves idle (profiles/r07c: config 3 at N = 8 0.200 -> 0.190 ms per slab, config 4
    2.42 -> 2.39; five and more lose again, and at N <= 4 and on one GPU three are best)."""
    return 4 if rank_count >= 8 else 3


def setup_config(scene, config, dataset, width=None, height=None, **overrides):
    """Applies one of the BASELINE.json configurations to a HostScene / Renderer."""
    from . import synthetic
    settings = dict(synthetic.CONFIG_SETTINGS[config])
    if width:
        settings["width"] = width
    if height:
        settings["height"] = height
    settings.update(overrides)
    wants_rays = bool(settings.get("trace_shadow_rays", False))
    # (a builder named by the caller wins; rays alone ask for the default builder)
    scene.load_scene(dataset["scene"], dataset["textures"], acceleration_structure=overrides.get("acceleration_structure") or wants_rays)
    scene.load_ltc_table(dataset["ltc"], dataset["fresnel_count"])
    scene.load_noise_table("white")
    cam = synthetic.DEFAULT_CAMERA
    scene.set_camera(cam["position"], cam["rotation_x"], cam["rotation_z"], cam["vertical_fov"], cam["near"], cam["far"])
    scene.set_lights(synthetic.config_lights(config))
    settings.pop("acceleration_structure", None)
    scene.set_settings(**settings)
    return settings
