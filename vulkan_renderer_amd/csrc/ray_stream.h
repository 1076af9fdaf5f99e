// What the tracing kernels (wavefront_kernels.h) and the replay that counts their work (traversal_statistics.hip) read: the
// queues that the shading kernel filled (shade_params has the same pointers, writable).  A header of its own because
// wavefront_kernels.h defines non-template kernels and so belongs to one unit alone.
#pragma once
#include "device_types.h"

namespace vkr {

struct ray_stream {
	const float4* directions;   // [queue][slot]: direction, t_max
	const uint32_t* records;    // [queue][slot]: thread | code cursor << thread_bits, or kNullRay
	const float4* origins;      // [thread]: where all rays of that pixel start
	const uint32_t* sizes;      // slots used per queue
	uint32_t capacity, thread_bits, thread_count;
};

}  // namespace vkr
