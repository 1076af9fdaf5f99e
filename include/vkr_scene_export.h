/* Export of meshes to *.vks scenes on the device: reference tools/io_export_vulkan_blender28.py:458-531. */
#ifndef VKR_SCENE_EXPORT_H
#define VKR_SCENE_EXPORT_H
#include "vkr_device.h"

/*! A triangle mesh in host memory, as the add-on's Mesh holds it: attributes per vertex, texture coordinates per
	triangle corner, one material slot per triangle */
typedef struct scene_export_source_s {
	uint64_t vertex_count, triangle_count, material_count;
	const float* vertex_positions;   /* 3 per vertex */
	const float* vertex_normals;     /* 3 per vertex */
	const uint32_t* vertex_indices;  /* 3 per triangle; NULL: triangle t uses vertices 3t, 3t+1, 3t+2 */
	const float* corner_tex_coords;  /* 2 per triangle corner; NULL: all zero */
	const uint8_t* material_indices; /* 1 per triangle; NULL: all zero */
	const char* const* material_names;
} scene_export_source_t;

/*! What a *.vks file holds (reference src/scene.c:77-150, csrc/host/scene.c) */
typedef struct exported_scene_s {
	uint64_t material_count, triangle_count;
	char** material_names;
	float dequantization_factor[3], dequantization_summand[3];
	uint32_t* positions;              /* 2 per corner, host memory */
	uint16_t* normals_and_tex_coords; /* 4 per corner */
	uint8_t* material_indices;        /* 1 per triangle */
} exported_scene_t;

/* export_scene() quantises, packs and (sort_triangles != 0) sorts the mesh on the device (HIP kernels of
   csrc/scene_export.hip on device->stream: one upload of the source arrays, one read-back) and returns 0.  It returns 1
   after printing one line, with the struct zeroed, for: device == NULL (there is no host build of the exporter),
   triangle_count == 0, 3 * triangle_count > 2^31 - 1, material_count outside 1 ... 256, a missing array or name, a vertex
   index >= vertex_count, a material index >= material_count, and a position, normal or texture coordinate that is not
   finite.  The last three are found on the device - the kernels raise bits of a flag word that the host reads - and an
   index is checked before it is used.  The rules that follow, the order of operations included, are the interface: the
   numpy restatement vulkan_renderer_amd/scene_export.py gives the same bytes.  They are the add-on's :458-528 operation
   for operation, as numpy 2 evaluates them; the fixtures of tests/golden/scene_export.npz are files the add-on wrote.
   Everything is binary32 unless stated, every multiplication and addition is rounded on its own, divisions are correctly
   rounded.  trunc() below converts to an unsigned integer towards zero.

   Box.  lo, hi are the minimum and maximum per axis over all vertex_count positions; vertices that no triangle uses
   count, as in the add-on.

   Quantisation (:477-487).  qf = 2097152.0f / (hi - lo), qo = -lo * qf, q = min(trunc(v * qf + qo), 2^21 - 1) per axis.
   dequantization_factor = 1.0f / qf, dequantization_summand = lo + 0.5f * dequantization_factor.

   Position packing (:499-506).  Word 0 = qx + ((qy & 0x7FF) << 21), word 1 = ((qy & 0x1FF800) >> 11) + (qz << 10); the
   two words of a corner are those of its vertex.

   Normals (:24-46).  l = (|x| + |y|) + |z|, o = (x / l, y / l).  If z <= 0 (so also for -0): o = ((1.0f - |o.y|) * s.x,
   (1.0f - |o.x|) * s.y) with s = +1 where the component of the unfolded o is >= 0 (so also for -0), else -1, all of it in
   binary32.  Then o is widened to binary64 and the code is (uint16_t) trunc(o * 32767.0 + 32768.5), the multiplication
   and the addition in binary64.  (numpy's promotion rules make the add-on do this.  Folding in binary64, or multiplying
   in binary32, changes about 4 normals in 10 000 by one code.)

   Texture coordinates (:510-520).  Per triangle and component m = floor(minimum over the three corners), uv -= m, and
   the code is (uint16_t) trunc(min(max(uv * 8191.875f + 0.5f, 0.0f), 65535.0f)): up to eight repetitions of a texture
   within a triangle, beyond that the coordinates are clipped.

   Sort (:459-469, 49-77; sort_triangles != 0).  The centroid is c = ((p0 + p1) + p2) / 3.0f per axis, clo and chi are the
   extremes of the centroids, f = 1024.0f / (chi - clo), g = trunc(min(max(c * f + (-clo * f), 0.0f), 1023.0f)), and
   code = spread(g.x) | spread(g.y) << 1 | spread(g.z) << 2, where spread() puts two zero bits between any two of the low
   ten bits: x is the LOWEST bit (the BVH builder csrc/bvh_build.hip and synthetic.write_vks have it the other way
   round).  Triangles are stored in ascending order of the code, and triangles of equal code keep their input order.
   (This is the project's rule: the add-on calls an unstable argsort, so its order among equal codes depends on the numpy
   build.)  Corners, texture coordinates and material indices move with their triangle.

   Rules of this project where the add-on divides by zero or leaves the result open.  An axis with hi == lo takes
   qf = qo = 0, dequantization_factor 0 and dequantization_summand lo; the same holds for the centroid box (f = 0 and
   the summand 0).  Zeros of lo, clo and dequantization_summand are stored as +0 (the minimum of -0 and +0 is either).  A
   normal with l == 0 has the code (32768, 32768).

   Material names (:489-490).  Copied after the add-on's two substitutions: a trailing '.' with three decimal digits is
   dropped, then every ".DoubleSided" is removed in one pass from the left.  Lengths are counted in bytes. */
VKR_API int export_scene(exported_scene_t* out, const device_t* device, const scene_export_source_t* source, VkBool32 sort_triangles);
/*! The container of export_scene() in the add-on (:470-531), which csrc/host/scene.c reads: uint32_t 0x00abcabc and 1,
	uint64_t material and triangle count, three floats factor and three floats summand, per name its uint64_t length, its
	bytes and a 0 byte, the positions, the normals and texture coordinates, the material indices, uint32_t 0x00e0fe0f.
	Returns 0 on success, 1 after printing one line */
VKR_API int write_exported_scene(const exported_scene_t* scene, const char* file_path);
VKR_API void free_exported_scene(exported_scene_t* scene);

/*! Milliseconds the kernels of the most recent successful export_scene() of this process took on the device, between two
	events on device->stream around them (the upload in front and the read-back behind are outside); 0 before the first */
VKR_API float get_scene_export_kernel_milliseconds(void);

#endif
