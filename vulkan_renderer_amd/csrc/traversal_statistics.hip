// Diagnostics (get_traversal_statistics*): replays the rays that the last frame queued and counts the work of the traversal
// (profiles/ and the tests cite these numbers; not part of the frame).  The replay walks with the pieces of a visit that
// the tracing kernels walk with (lbvh.h: threaded_next, visit_wide_node, leaf_triangle), so it counts what they do.
#include "frame_pipeline.h"
#include "lbvh.h"
#include "ray_stream.h"

using namespace vkr;

// What one ray's walk cost: fetched nodes (dependent loads) and triangle tests; on the wide tree also the tested boxes of
// children that exist and the deepest stack the ray reached
struct ray_work { uint32_t visits = 0, tests = 0, boxes = 0, deepest = 0; bool blocked = false; };

// trace_shadow_rays: the threaded binary tree
VKR_DEV ray_work walk_binary(const bvh_view& bvh, f3 o, f3 d, float t_max) {
	ray_work w;
	grid_ray ray = make_grid_ray(bvh, o, d);
	uint32_t node = 0;
	while (t_max >= 1.0e-3f && node < bvh.node_count && !w.blocked) {
		uint4 n = bvh.nodes[node];
		bool hit = ray_box(n, ray, 1.0e-3f, t_max);
		++w.visits;
		if (hit && (n.w & kLeafBit) != 0) {
			const float4* t = leaf_triangle(bvh, n.w);
			float dist;
			++w.tests;
			w.blocked = ray_triangle<false>(t[0], t[1], t[2], o, d, 1.0e-3f, t_max, dist);
		}
		node = threaded_next(node, n, hit);
	}
	return w;
}

// trace_shadow_rays_wide: the four-wide tree, the children of a node in its order - child 0 next, then 1, 2, 3 (pushed last
// to first).  The next item is kept apart from the stack here; the tracing kernel holds it on the stack too, one entry more.
VKR_DEV ray_work walk_wide(const bvh_view& bvh, const uint4* wide_nodes, f3 o, f3 d, float t_max) {
	constexpr uint32_t kNone = 0xFFFFFFFFu;  // no next item: take one off the stack
	ray_work w;
	wide_ray ray = make_wide_ray(make_grid_ray(bvh, o, d));
	uint32_t stack[kWideStackMax];
	uint32_t depth = 0, item = 0;
	while (t_max >= 1.0e-3f) {
		if (item & kLeafBit) {
			const float4* t = leaf_triangle(bvh, item);
			float dist;
			++w.tests;
			w.blocked = ray_triangle<false>(t[0], t[1], t[2], o, d, 1.0e-3f, t_max, dist);
			if (w.blocked) break;
			item = kNone;
		}
		else {
			const wide_visit v = visit_wide_node(wide_nodes, item, ray, 1.0e-3f, t_max);
			const uint32_t links[4] = {v.link.x, v.link.y, v.link.z, v.link.w};
			++w.visits;
			item = kNone;
			for (int c = 3; c >= 0; --c) {
				if (links[c] == kWideEmpty) continue;
				++w.boxes;
				if (!v.hit[c]) continue;
				if (item != kNone && depth < kWideStackMax) stack[depth++] = item;
				item = links[c];
			}
			w.deepest = max(w.deepest, depth);
		}
		if (item == kNone) {
			if (depth == 0) break;
			item = stack[--depth];
		}
	}
	return w;
}

// `walk(o, d, t_max)` for every queued ray, 64 consecutive slots of a queue per wave like a batch of the tracing kernels.
// out[0] rays, [1] node visits, [2] triangle tests, [3] blocked rays, [4] wave steps - the longest ray of each 64 -, [5] the
// longest ray's visits; of a walk WITH_STACK also [6] tested boxes, [7] the deepest stack, [8] the rays whose stack outgrows the
// `lds_entries` that trace_shadow_rays_wide keeps in LDS, [9] the node visits of the rays that end up blocked.
template <bool WITH_STACK, typename walk_t>
VKR_DEV void replay_queued_rays(const ray_stream& stream, uint32_t lds_entries, unsigned long long* out, walk_t walk) {
	const uint32_t queue = blockIdx.y, size = stream.sizes[queue];
	unsigned long long visits = 0, tests = 0, blocked_rays = 0, rays = 0, wave_steps = 0, boxes = 0, beyond_lds = 0, blocked_visits = 0;
	for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < ((size + 63u) & ~63u); i += gridDim.x * 256u) {
		ray_work mine;
		size_t slot = (size_t) queue * stream.capacity + i;
		// (a slot that the shading wave reserved and did not need holds kNullRay)
		if (i < size && stream.records[slot] != kNullRay) {
			float4 a = stream.origins[ray_record_thread(stream.thread_bits, stream.records[slot])], b = stream.directions[slot];
			mine = walk(mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), b.w);
			++rays;
			tests += mine.tests; boxes += mine.boxes;
			blocked_rays += mine.blocked ? 1 : 0;
			blocked_visits += mine.blocked ? mine.visits : 0u;
			beyond_lds += (mine.deepest + 1u > lds_entries) ? 1 : 0;
			if (WITH_STACK) atomicMax(out + 7, (unsigned long long) mine.deepest);
		}
		visits += mine.visits;
		// steps the wave needs for these 64 rays = longest ray
		uint32_t longest = mine.visits;
		for (int offset = 32; offset > 0; offset >>= 1) longest = max(longest, (uint32_t) __shfl_xor((int) longest, offset));
		if ((threadIdx.x & 63u) == 0) wave_steps += longest;
		atomicMax(out + 5, (unsigned long long) mine.visits);
	}
	atomicAdd(out + 0, rays); atomicAdd(out + 1, visits); atomicAdd(out + 2, tests);
	atomicAdd(out + 3, blocked_rays); atomicAdd(out + 4, wave_steps);
	if (WITH_STACK) {
		atomicAdd(out + 6, boxes);
		if (beyond_lds) atomicAdd(out + 8, beyond_lds);
		if (blocked_visits) atomicAdd(out + 9, blocked_visits);
	}
}

__global__ void __launch_bounds__(256) k_traversal_statistics(bvh_view bvh, ray_stream stream, unsigned long long* out) {
	replay_queued_rays<false>(stream, 0u, out, [&](f3 o, f3 d, float t_max) { return walk_binary(bvh, o, d, t_max); });
}

__global__ void __launch_bounds__(256) k_traversal_statistics_wide(bvh_view bvh, const uint4* wide_nodes, ray_stream stream, uint32_t lds_entries, unsigned long long* out) {
	replay_queued_rays<true>(stream, lds_entries, out, [&](f3 o, f3 d, float t_max) { return walk_wide(bvh, wide_nodes, o, d, t_max); });
}

extern "C" int get_traversal_statistics(application_t* app, uint64_t out_statistics[6]) {
	const wavefront_buffers* w = last_launch_buffers(app);
	if (!w || !w->ray_directions || !app->shading_pass.use_ray_tracing || app->shading_pass.inline_rays) {
		printf("get_traversal_statistics() needs a frame rendered with wavefront shadow rays.\n");
		return 1;
	}
	uint64_t all[12];
	int failed = get_traversal_statistics_of_tree(app, app->scene.acceleration_structure.wide_nodes && !app->shading_pass.binary_traversal, all);
	memcpy(out_statistics, all, sizeof(uint64_t) * 6);
	return failed;
}

extern "C" int get_traversal_statistics_of_tree(application_t* app, VkBool32 wide_tree, uint64_t out_statistics[12]) {
	const frame_pipeline* frames = (const frame_pipeline*) app->shading_pass.wavefront;
	const wavefront_buffers* w = last_launch_buffers(app);
	const acceleration_structure_t* structure = &app->scene.acceleration_structure;
	if (!w || !w->ray_directions || !app->shading_pass.use_ray_tracing || app->shading_pass.inline_rays || (wide_tree && !structure->wide_nodes)) {
		printf("get_traversal_statistics_of_tree() needs a frame rendered with wavefront shadow rays (and the tree it is asked about).\n");
		return 1;
	}
	unsigned long long* counters = NULL;
	if (hip_failed(hipMalloc(&counters, sizeof(unsigned long long) * 12), "allocating traversal counters")) return 1;
	hipStream_t stream = (hipStream_t) app->device.stream;
	(void) finish_frames(app);
	(void) hipMemsetAsync(counters, 0, sizeof(unsigned long long) * 12, stream);
	bvh_view bvh = make_bvh_view(structure);
	// (the queues of the most recent launch - the last band of the last frame - with the sizes the resolve kernel kept)
	ray_stream rays = {w->ray_directions, w->ray_records, w->ray_origins, w->ray_queue_size + kRayCounterCount, w->queue_capacity, w->thread_bits, w->thread_count};
	if (wide_tree) k_traversal_statistics_wide<<<dim3(16, kRayQueueCount), 256, 0, stream>>>(bvh, (const uint4*) structure->wide_nodes, rays, frames->wide_stack_lds, counters);
	else k_traversal_statistics<<<dim3(16, kRayQueueCount), 256, 0, stream>>>(bvh, rays, counters);
	int failed = vkr_copy_to_host(out_statistics, counters, sizeof(uint64_t) * 12, &app->device);
	(void) hipFree(counters);
	return failed;
}
