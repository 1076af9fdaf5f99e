// What a kernel is given of a built BVH (layout and traversal: lbvh.h), apart from the traversal code so that the launch
// contract (shade_params.h) can hold one, and how the host fills it from a scene's acceleration structure.
#pragma once
#include "device_types.h"
#include "vkr_scene.h"

namespace vkr {

struct bvh_view {
	const uint4* nodes;       // 16 bytes per node, depth-first order
	const float4* triangles;  // 3 float4 per leaf slot
	uint32_t node_count;      // 2 * triangle_count - 1
	f3 grid_origin, grid_inverse_cell;
};

inline bvh_view make_bvh_view(const acceleration_structure_t* structure) {
	bvh_view view;
	view.nodes = (const uint4*) structure->nodes;
	view.triangles = (const float4*) structure->triangle_vertices;
	view.node_count = structure->node_count;
	view.grid_origin = f3{structure->grid_origin[0], structure->grid_origin[1], structure->grid_origin[2]};
	view.grid_inverse_cell = f3{structure->grid_inverse_cell[0], structure->grid_inverse_cell[1], structure->grid_inverse_cell[2]};
	return view;
}

}  // namespace vkr
