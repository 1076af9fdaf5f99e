// What a kernel is given of a built BVH (layout and traversal: lbvh.h), apart from the traversal code so that the launch
// contract (shade_params.h) can hold one.
#pragma once
#include "device_types.h"

namespace vkr {

struct bvh_view {
	const uint4* nodes;       // 16 bytes per node, depth-first order
	const float4* triangles;  // 3 float4 per leaf slot
	uint32_t node_count;      // 2 * triangle_count - 1
	f3 grid_origin, grid_inverse_cell;
};

}  // namespace vkr
