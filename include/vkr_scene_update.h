/* Moving geometry: new vertex positions for the mesh of a loaded scene, and the acceleration structure brought up to
   date by a refit (csrc/bvh_refit.hip) or a rebuild.  No reference counterpart: the reference builds its acceleration
   structure once and never touches it again (src/scene.c:142-406). */
#ifndef VKR_SCENE_UPDATE_H
#define VKR_SCENE_UPDATE_H
#include "vkr_scene.h"

/*! How update_scene_geometry() brings the tree up to date.  No reference counterpart (src/scene.c:142-406 builds once). */
typedef enum scene_update_policy_e {
	/*! keep the topology of both layouts, recompute every box bottom-up */
	scene_update_refit = 0,
	/*! destroy the structure and build it again with the builder that made it */
	scene_update_rebuild,
	/*! refit, measure the cost of the refitted tree, and rebuild if it exceeds rebuild_above times the cost as built */
	scene_update_auto
} scene_update_policy_t;

/*! No reference counterpart (src/scene.c:142-406 builds once). */
typedef struct scene_update_options_s {
	/*! a scene_update_policy_t */
	uint32_t policy;
	/*! positions / normals_and_tex_coords are device pointers, else host pointers */
	VkBool32 inputs_on_device;
	/*! keep mesh.host_positions (and host_normals_and_tex_coords) equal to the device arrays; a rebuild with the host
		builder reads them */
	VkBool32 refresh_host_copy;
	/*! fill scene_update_report_t.cost and built_cost */
	VkBool32 measure_cost;
	/*! scene_update_auto: rebuild when cost / built_cost exceeds this; 0: never */
	float rebuild_above;
} scene_update_options_t;

/*! No reference counterpart (src/scene.c:142-406 builds once). */
typedef struct scene_update_report_s {
	/*! 1 if the call ended in a full build */
	uint32_t rebuilt;
	/*! the structure's new build_serial (0 for a scene without acceleration structure) */
	uint32_t build_serial;
	/*! device time of the update between two HIP events on device->stream (a rebuild: with its host synchronisations) */
	float milliseconds;
	/*! Cost of the refitted tree and of the tree as built: the sum over the inner nodes of the binary tree of the half-area
		ex ey + ey ez + ez ex of their quantised boxes, in world units.  The three sums of products are exact integers in grid
		cells; cost = (double) sum_xy * (cx * cy) + (double) sum_yz * (cy * cz) + (double) sum_zx * (cz * cx) with the cell
		sizes c = 1.0 / (double) grid_inverse_cell, evaluated in binary64 from left to right, nothing contracted.  A surface
		area heuristic without the leaves: what grows when boxes of a refitted tree begin to overlap.  0 unless measured. */
	double cost, built_cost;
} scene_update_report_t;

/*! Replaces the vertex positions of scene->mesh (and its normals and texture coordinates unless that pointer is NULL)
	and brings the acceleration structure, if the scene has one, up to date.  No reference counterpart: its tree is built
	once (src/scene.c:142-406).

	positions has the layout of the scene file: 2 uint32_t per vertex (21 bits per coordinate, vkr_scene.h), 3 vertices per
	triangle, mesh.triangle_count triangles; normals_and_tex_coords 4 uint16_t per vertex.  The codes live in the
	mesh's unchanged de-quantisation box; triangle count and order, material indices and the de-quantisation constants
	do not change.  options NULL: refit, host pointers, refreshed host copy, no cost.

	The arrays replace mesh.positions / mesh.normals_and_tex_coords in place.  triangle_vertices, nodes and wide_nodes
	keep their allocation, their topology and every link; their vertices and boxes become those of the moved mesh, on a
	grid chosen from the moved mesh's box exactly as a build chooses it, so geometry may move anywhere inside the
	de-quantisation box.  A leaf of a split triangle covers the same slab j of count of the moved triangle, along the
	longest axis of its new box.  build_serial gets a fresh value from the counter of the builds: whatever the shading
	pass keeps per tree is not kept across an update.  A rebuild (scene_update_rebuild, or scene_update_auto above its
	threshold) destroys the structure and builds it again with acceleration_structure_t.builder.

	The call synchronises the HIP device before its first write and returns once the update is complete on
	device->stream.  A caller with frames in flight calls finish_frames() first, and render_visibility_pass()
	afterwards: the visibility buffer still names the triangles that were visible before.

	Returns 0 on success.  Returns 1 after printing one line, with the scene as it was, for scene, device or positions
	NULL, a policy that is no scene_update_policy_t and a negative or NaN rebuild_above.  A HIP error on the way also
	returns 1; the scene is then in an unspecified state and only good for destroy_scene(). */
VKR_API int update_scene_geometry(scene_t* scene, const device_t* device, const uint32_t* positions,
                                  const uint16_t* normals_and_tex_coords, const scene_update_options_t* options,
                                  scene_update_report_t* out_report);

#endif
