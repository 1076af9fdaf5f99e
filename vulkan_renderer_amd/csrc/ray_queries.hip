// Ray queries for the caller's rays (include/vkr_ray_queries.h trace_closest_hits, trace_any_hits): one lane per ray,
// on the threaded binary tree or on the four-wide tree of lbvh.h.  The tree only culls; which triangle wins is decided by
// the rules of the header, which the numpy restatement (vulkan_renderer_amd/ray_queries.py) repeats bit for bit.  Compiled
// without contraction and with correctly rounded divisions; there is one build of this unit, whatever the arithmetic
// mode of the shading pass.
#include "vkr_ray_queries.h"
#include "host/vkr_internal.h"
#include "lbvh.h"
#include <hip/hip_runtime.h>
#include <map>
#include <mutex>

using namespace vkr;

constexpr uint32_t kBlock = 256;
// Boxes are tested against the ray's interval widened by this fraction of either end (on top of the outward rounding of
// the quantised boxes, kGridMargin): t = T / adet of a triangle that passes is off its geometric value by a few 2^-24
// of t over the cosine of the angle of incidence, and a box that the exact intersection lies in must not be culled by
// the rounded t of another triangle - or by the ray's own t_min or t_max.  2^-10 covers cosines down to about 2^-10
// (the bound that the header states); what it costs in box tests was not measured.
constexpr float kWiden = 0x1.0p-10f;
// The slab test is exact enough for the margin of the boxes only while the origin is within this many cells of the grid
// (the grid has 2^15 across the scene box: the origin's grid coordinate is off by about 2^-23 of itself, 0.01 cells here,
// against kGridMargin = 0.05) and the direction's reciprocal neither overflows nor vanishes.  Rays outside these bounds,
// infinite components included, are tested against every triangle: the tree may only cull what the triangle test rejects.
constexpr float kFarthestOriginInCells = 0x1.0p16f, kLargestDirection = 0x1.0p60f, kSmallestDirection = 0x1.0p-60f;

struct query_ray {
	f3 o, d;
	float t_min, t_max;
	// rule 6 of the header: no triangle can pass
	bool misses;
	// every box counts as hit
	bool no_culling;
};

__device__ static inline query_ray load_ray(const ray_t* rays, uint32_t index) {
	const float4* words = (const float4*) (rays + index);
	float4 a = words[0], b = words[1];
	query_ray r;
	r.o = mk3(a.x, a.y, a.z); r.t_min = a.w;
	r.d = mk3(b.x, b.y, b.z); r.t_max = b.w;
	float sum = ((a.x + a.y) + (a.z + a.w)) + ((b.x + b.y) + (b.z + b.w));
	// (a sum of infinities of both signs is NaN as well: such a ray is looked at again component by component)
	bool has_nan = sum != sum && (a.x != a.x || a.y != a.y || a.z != a.z || a.w != a.w || b.x != b.x || b.y != b.y || b.z != b.z || b.w != b.w);
	r.misses = has_nan || !(r.t_max >= r.t_min) || (b.x == 0.0f && b.y == 0.0f && b.z == 0.0f);
	r.no_culling = false;
	return r;
}

__device__ static inline bool cannot_cull(const bvh_view& bvh, const query_ray& r) {
	float ox = (r.o.x - bvh.grid_origin.x) * bvh.grid_inverse_cell.x, oy = (r.o.y - bvh.grid_origin.y) * bvh.grid_inverse_cell.y, oz = (r.o.z - bvh.grid_origin.z) * bvh.grid_inverse_cell.z;
	float farthest = fmaxf(fmaxf(fabsf(ox), fabsf(oy)), fabsf(oz));
	float dx = fabsf(r.d.x), dy = fabsf(r.d.y), dz = fabsf(r.d.z);
	float largest = fmaxf(fmaxf(dx, dy), dz);
	// (written so that NaNs and infinities end up here)
	return !(farthest <= kFarthestOriginInCells) || !(largest <= kLargestDirection) || !(largest >= kSmallestDirection);
}

// the far and the near end of the interval that boxes are tested against
__device__ static inline float widened_far(float t_max, float best) {
	float far = fminf(t_max, best);
	return far + fabsf(far) * kWiden;
}
__device__ static inline float widened_near(float t_min) { return t_min - fabsf(t_min) * kWiden; }

// (t, primitive) in lexicographic order, a NaN above every number
__device__ static inline bool hit_wins(float t, uint32_t primitive, float best_t, uint32_t best_primitive) {
	bool less = t < best_t || (best_t != best_t && t == t);
	bool same = t == best_t || (t != t && best_t != best_t);
	return less || (same && primitive < best_primitive);
}

// The best hit so far and the triangle test that may replace it.  The test is ray_triangle<CULL_BACK>() of lbvh.h with the
// ray's own interval; the values of a hit repeat its operations (the compiler merges them with the test's).
struct closest_hit {
	uint32_t primitive;
	float t, u, v;
};

template <bool CULL_BACK>
__device__ static inline void test_leaf(const bvh_view& bvh, uint32_t link, const query_ray& r, closest_hit& best) {
	const float4* t = leaf_triangle(bvh, link);
	float4 p0 = t[0], p1 = t[1], p2 = t[2];
	float unused;
	if (!ray_triangle<CULL_BACK>(p0, p1, p2, r.o, r.d, r.t_min, r.t_max, unused)) return;
	f3 e1 = mk3(p1.x - p0.x, p1.y - p0.y, p1.z - p0.z);
	f3 e2 = mk3(p2.x - p0.x, p2.y - p0.y, p2.z - p0.z);
	f3 p = cross(r.d, e2);
	float det = dot(e1, p);
	float sign = (det < 0.0f) ? -1.0f : 1.0f;
	float adet = det * sign;
	f3 s = mk3(r.o.x - p0.x, r.o.y - p0.y, r.o.z - p0.z);
	float U = dot(s, p) * sign;
	f3 q = cross(s, e1);
	float V = dot(r.d, q) * sign;
	float T = dot(e2, q) * sign;
	float dist = T / adet;
	uint32_t primitive = __float_as_uint(p0.w);
	if (hit_wins(dist, primitive, best.t, best.primitive)) {
		best.primitive = primitive;
		best.t = dist; best.u = U / adet; best.v = V / adet;
	}
}

__device__ static inline void store_hit(ray_hit_t* out, uint32_t index, const closest_hit& best) {
	*(uint4*) (out + index) = make_uint4(best.primitive, __float_as_uint(best.t), __float_as_uint(best.u), __float_as_uint(best.v));
}

// rule 4 of the header
__device__ static inline closest_hit miss() { return closest_hit{0xFFFFFFFFu, __builtin_inff(), 0.0f, 0.0f}; }

// ---- the threaded binary tree: a cursor, no stack -------------------------------------------------------------------

template <bool CULL_BACK>
__global__ void __launch_bounds__(kBlock) k_closest_hits_binary(bvh_view bvh, const ray_t* __restrict__ rays, uint32_t count, ray_hit_t* __restrict__ out_hits) {
	uint32_t index = blockIdx.x * kBlock + threadIdx.x;
	if (index >= count) return;
	query_ray r = load_ray(rays, index);
	r.no_culling = cannot_cull(bvh, r);
	closest_hit best = miss();
	if (!r.misses) {
		grid_ray g = make_grid_ray(bvh, r.o, r.d);
		const float near = widened_near(r.t_min);
		uint32_t node = 0;
		const uint32_t end = bvh.node_count;
		while (node < end) {
			uint4 n = bvh.nodes[node];
			bool is_leaf = (n.w & kLeafBit) != 0;
			bool hit = r.no_culling || ray_box(n, g, near, widened_far(r.t_max, best.t));
			if (hit && is_leaf) test_leaf<CULL_BACK>(bvh, n.w, r, best);
			node = threaded_next(node, n, hit);
		}
	}
	store_hit(out_hits, index, best);
}

__global__ void __launch_bounds__(kBlock) k_any_hits_binary(bvh_view bvh, const ray_t* __restrict__ rays, uint32_t count, uint8_t* __restrict__ out_blocked) {
	uint32_t index = blockIdx.x * kBlock + threadIdx.x;
	if (index >= count) return;
	query_ray r = load_ray(rays, index);
	r.no_culling = cannot_cull(bvh, r);
	bool blocked = false;
	if (!r.misses) {
		grid_ray g = make_grid_ray(bvh, r.o, r.d);
		const float near = widened_near(r.t_min), far = widened_far(r.t_max, r.t_max);
		uint32_t node = 0;
		const uint32_t end = bvh.node_count;
		float unused;
		while (node < end) {
			uint4 n = bvh.nodes[node];
			bool is_leaf = (n.w & kLeafBit) != 0;
			bool hit = r.no_culling || ray_box(n, g, near, far);
			if (hit && is_leaf) {
				const float4* t = leaf_triangle(bvh, n.w);
				if (ray_triangle<false>(t[0], t[1], t[2], r.o, r.d, r.t_min, r.t_max, unused)) { blocked = true; break; }
			}
			node = threaded_next(node, n, hit);
		}
	}
	out_blocked[index] = blocked ? 1 : 0;
}

// ---- the four-wide tree: a stack per lane ---------------------------------------------------------------------------

// The stack of a lane: `lds_entries` links [entry][thread] in LDS (a per-lane slot never conflicts on banks), deeper ones
// [entry][thread of the grid] in `spill`, which the host sizes from the worst case of the build
// (acceleration_structure_t.wide_stack_need): a stack cannot outgrow it.  A link is that of a wide node: an inner
// node's index or kLeafBit | triangle slot.  (LDS through lds_u32 of lbvh.h.)
struct lane_stack {
	uint32_t lds_links;
	uint32_t* spill_links;
	size_t spill_stride;
	uint32_t lds_entries, top;

	__device__ inline void push(uint32_t link) {
		if (top < lds_entries) *(lds_u32*) (uintptr_t) (lds_links + top * (kBlock * 4u)) = link;
		else spill_links[(size_t) (top - lds_entries) * spill_stride] = link;
		++top;
	}
	__device__ inline uint32_t pop() {
		--top;
		if (top < lds_entries) return *(lds_u32*) (uintptr_t) (lds_links + top * (kBlock * 4u));
		return spill_links[(size_t) (top - lds_entries) * spill_stride];
	}
};

// (kWideStackLds = 16 links per lane are 16 KB per workgroup, thirteen of the 1280-byte granules in which gfx950 hands out
// LDS: eight workgroups, i.e. all 32 waves, fit a CU)
__device__ static inline lane_stack make_lane_stack(uint32_t* lds, uint32_t* spill, uint32_t lds_entries) {
	lane_stack stack;
	stack.lds_links = (uint32_t) (uintptr_t) (lds_u32*) (lds + threadIdx.x);
	stack.spill_stride = (size_t) gridDim.x * kBlock;
	stack.spill_links = spill + (size_t) blockIdx.x * kBlock + threadIdx.x;
	stack.lds_entries = lds_entries;
	stack.top = 0;
	return stack;
}

// swaps so that the first of the two children is the farther one (a child that was not hit counts as the farthest)
__device__ static inline void farther_first(float& distance_a, uint32_t& link_a, float& distance_b, uint32_t& link_b) {
	bool swap = distance_a < distance_b;
	float d = swap ? distance_b : distance_a, e = swap ? distance_a : distance_b;
	uint32_t l = swap ? link_b : link_a, m = swap ? link_a : link_b;
	distance_a = d; distance_b = e; link_a = l; link_b = m;
}

// Closest hit.  A visit fetches one 64-byte node, tests its four boxes against the interval that ends at the best hit so
// far and pushes the children that were hit, the farthest first, so that the nearest comes off the stack next and the
// hits shrink the interval early.  Measured against pushing in the order of the node, and against entries that carry the
// parameter at which the ray enters the box so that stale ones are dropped without a fetch: the ordered
// push won on every ray set, the distances lost on every one (they halve the entries that fit into LDS).
template <bool CULL_BACK>
__global__ void __launch_bounds__(kBlock) k_closest_hits_wide(bvh_view bvh, const uint4* __restrict__ wide_nodes, const ray_t* __restrict__ rays, uint32_t count, ray_hit_t* __restrict__ out_hits,
	uint32_t* spill, uint32_t lds_entries)
{
	__shared__ uint32_t lds[kWideStackLds * kBlock];
	uint32_t index = blockIdx.x * kBlock + threadIdx.x;
	if (index >= count) return;
	query_ray r = load_ray(rays, index);
	r.no_culling = cannot_cull(bvh, r);
	closest_hit best = miss();
	if (!r.misses) {
		wide_ray ray = make_wide_ray(make_grid_ray(bvh, r.o, r.d));
		const float near = widened_near(r.t_min);
		lane_stack stack = make_lane_stack(lds, spill, lds_entries);
		// the root
		uint32_t item = 0;
		while (true) {
			if (item & kLeafBit) test_leaf<CULL_BACK>(bvh, item, r, best);
			else {
				const wide_visit v = visit_wide_node(wide_nodes, item, ray, near, widened_far(r.t_max, best.t));
				float d0 = v.entry[0], d1 = v.entry[1], d2 = v.entry[2], d3 = v.entry[3];
				// (an absent child cannot be hit unless NaNs let it through: its link is never pushed)
				const bool h0 = v.hit[0] || r.no_culling, h1 = v.hit[1] || r.no_culling, h2 = v.hit[2] || r.no_culling, h3 = v.hit[3] || r.no_culling;
				uint32_t l0 = h0 ? v.link.x : kWideEmpty, l1 = h1 ? v.link.y : kWideEmpty, l2 = h2 ? v.link.z : kWideEmpty, l3 = h3 ? v.link.w : kWideEmpty;
				// (NaN distances of rays that are not culled order nothing, which is as good as any order)
				const float inf = __builtin_inff();
				d0 = (l0 != kWideEmpty) ? d0 : inf; d1 = (l1 != kWideEmpty) ? d1 : inf; d2 = (l2 != kWideEmpty) ? d2 : inf; d3 = (l3 != kWideEmpty) ? d3 : inf;
				farther_first(d0, l0, d1, l1); farther_first(d2, l2, d3, l3);
				farther_first(d0, l0, d2, l2); farther_first(d1, l1, d3, l3);
				farther_first(d1, l1, d2, l2);
				if (l0 != kWideEmpty) stack.push(l0);
				if (l1 != kWideEmpty) stack.push(l1);
				if (l2 != kWideEmpty) stack.push(l2);
				if (l3 != kWideEmpty) stack.push(l3);
			}
			if (stack.top == 0) break;
			item = stack.pop();
		}
	}
	store_hit(out_hits, index, best);
}

// Any hit: the same walk without order, which ends at the first triangle that passes
__global__ void __launch_bounds__(kBlock) k_any_hits_wide(bvh_view bvh, const uint4* __restrict__ wide_nodes, const ray_t* __restrict__ rays, uint32_t count, uint8_t* __restrict__ out_blocked,
	uint32_t* spill, uint32_t lds_entries)
{
	__shared__ uint32_t lds[kWideStackLds * kBlock];
	uint32_t index = blockIdx.x * kBlock + threadIdx.x;
	if (index >= count) return;
	query_ray r = load_ray(rays, index);
	r.no_culling = cannot_cull(bvh, r);
	bool blocked = false;
	if (!r.misses) {
		wide_ray ray = make_wide_ray(make_grid_ray(bvh, r.o, r.d));
		const float near = widened_near(r.t_min), far = widened_far(r.t_max, r.t_max);
		lane_stack stack = make_lane_stack(lds, spill, lds_entries);
		uint32_t item = 0;
		float unused;
		while (true) {
			if (item & kLeafBit) {
				const float4* t = leaf_triangle(bvh, item);
				if (ray_triangle<false>(t[0], t[1], t[2], r.o, r.d, r.t_min, r.t_max, unused)) { blocked = true; break; }
			}
			else {
				const wide_visit v = visit_wide_node(wide_nodes, item, ray, near, far);
				if ((v.hit[3] || r.no_culling) && v.link.w != kWideEmpty) stack.push(v.link.w);
				if ((v.hit[2] || r.no_culling) && v.link.z != kWideEmpty) stack.push(v.link.z);
				if ((v.hit[1] || r.no_culling) && v.link.y != kWideEmpty) stack.push(v.link.y);
				if ((v.hit[0] || r.no_culling) && v.link.x != kWideEmpty) stack.push(v.link.x);
			}
			if (stack.top == 0) break;
			item = stack.pop();
		}
	}
	out_blocked[index] = blocked ? 1 : 0;
}

// ---- host ------------------------------------------------------------------------------------------------------------

// What both calls check and decide: 0 and the walk in *walk (a ray_walk_t other than ray_walk_auto), or 1 after one line
static int plan_query(const char* call, const scene_t* scene, const device_t* device, uint64_t count, const ray_query_options_t* options, uint32_t* walk, uint32_t* lds_entries) {
	const acceleration_structure_t* structure = scene ? &scene->acceleration_structure : NULL;
	*walk = options ? options->walk : (uint32_t) ray_walk_auto;
	*lds_entries = options ? options->lds_stack_entries : 0u;
	if (!device) {
		printf("%s() traces rays on the device; a HIP device is required.\n", call);
		return 1;
	}
	if (!structure || !structure->nodes || !structure->triangle_vertices || !structure->node_count) {
		printf("%s() needs a scene that was loaded with an acceleration structure.\n", call);
		return 1;
	}
	if (count > ((uint64_t) 1 << 31)) {
		printf("%s() takes at most 2^31 rays per call, not %llu.\n", call, (unsigned long long) count);
		return 1;
	}
	if (*walk > (uint32_t) ray_walk_wide) {
		printf("%s() was given walk %u, which is no ray_walk_t.\n", call, *walk);
		return 1;
	}
	if (*lds_entries > kWideStackLds) {
		printf("%s() keeps at most %u stack entries per ray in LDS, not %u.\n", call, kWideStackLds, *lds_entries);
		return 1;
	}
	const bool has_wide_tree = structure->wide_nodes && structure->wide_stack_need <= kWideStackMax;
	if (*walk == ray_walk_auto) *walk = has_wide_tree ? ray_walk_wide : ray_walk_binary;
	else if (*walk == ray_walk_wide && !has_wide_tree) {
		if (!structure->wide_nodes) printf("%s() was asked to walk the four-wide tree of a scene that has none.\n", call);
		else printf("%s() was asked to walk a four-wide tree that needs a stack of %u entries per ray (at most %u are provided).\n", call, structure->wide_stack_need, kWideStackMax);
		return 1;
	}
	return 0;
}

// The stack entries beyond LDS: one buffer per HIP device, allocated by the first wide call that needs it, kept for the
// later ones (an allocation per call cost 0.05 - 0.10 ms, more than the walk of two million coherent rays), grown on
// demand and freed by destroy_hip_device().  A launch uses at most kMostSpillBytes of it: more rays are traced in several
// launches, one after the other.  Calls share the buffer, so they are ordered on the device: a call on another stream
// than the last one waits there for the event that the last one recorded behind its kernels; the mutex is held from that
// wait to the next record, so that calls of several host threads cannot interleave.
constexpr size_t kMostSpillBytes = (size_t) 256 << 20;
struct spill_buffer {
	uint32_t* memory = NULL;
	size_t bytes = 0;
	hipEvent_t last_use = NULL;
	hipStream_t last_stream = NULL;
};
static std::mutex spill_mutex;
static std::map<int32_t, spill_buffer> spill_buffers;

extern "C" void vkr_free_ray_query_buffers(int32_t hip_device) {
	std::lock_guard<std::mutex> lock(spill_mutex);
	auto found = spill_buffers.find(hip_device);
	if (found == spill_buffers.end()) return;
	// (hipFree waits for the kernels that still use the memory)
	(void) hipFree(found->second.memory);
	if (found->second.last_use) (void) hipEventDestroy(found->second.last_use);
	spill_buffers.erase(found);
}

// Runs launch(first ray, ray count, spill buffer) over the rays: in one piece without a buffer if the stack of the wide walk
// fits into LDS, else in pieces that share the device's buffer
template <typename launch_t>
static int launch_wide(const char* call, const acceleration_structure_t* structure, const device_t* device, uint64_t count, uint32_t lds_entries, hipStream_t stream, launch_t launch) {
	const uint32_t spill_entries = structure->wide_stack_need > lds_entries ? structure->wide_stack_need - lds_entries : 0u;
	if (!spill_entries) {
		launch((uint64_t) 0, count, (uint32_t*) NULL);
		return hip_failed(hipGetLastError(), call);
	}
	// (spill_entries <= kWideStackMax: a piece is never empty)
	const size_t bytes_per_ray = sizeof(uint32_t) * spill_entries;
	uint64_t piece = (kMostSpillBytes / bytes_per_ray) / kBlock * kBlock;
	if (piece > count) piece = (count + kBlock - 1) / kBlock * kBlock;
	std::lock_guard<std::mutex> lock(spill_mutex);
	spill_buffer& buffer = spill_buffers[device->hip_device];
	if (!buffer.last_use && hip_failed(hipEventCreateWithFlags(&buffer.last_use, hipEventDisableTiming), "creating the event of the stack entries beyond LDS")) return 1;
	if (buffer.bytes < bytes_per_ray * piece) {
		// (hipFree waits for the kernels that still use the memory)
		(void) hipFree(buffer.memory);
		buffer.memory = NULL; buffer.bytes = 0;
		if (hipMalloc(&buffer.memory, bytes_per_ray * piece) != hipSuccess) {
			printf("Failed to allocate %.1f MiB for the traversal stacks of %s() that do not fit into LDS.\n", bytes_per_ray * piece / 1048576.0, call);
			return 1;
		}
		buffer.bytes = bytes_per_ray * piece;
		buffer.last_stream = stream;
	}
	if (buffer.last_stream != stream && hip_failed(hipStreamWaitEvent(stream, buffer.last_use, 0), "waiting for the ray query before")) return 1;
	for (uint64_t first = 0; first < count; first += piece)
		launch(first, (count - first < piece) ? count - first : piece, buffer.memory);
	int failed = hip_failed(hipGetLastError(), call);
	buffer.last_stream = stream;
	return hip_failed(hipEventRecord(buffer.last_use, stream), "recording the end of the ray query") | failed;
}

template <bool CULL_BACK>
static int launch_closest_hits(const scene_t* scene, const device_t* device, uint32_t walk, uint32_t lds_option, const ray_t* rays, uint64_t count, ray_hit_t* out_hits, hipStream_t stream) {
	const acceleration_structure_t* structure = &scene->acceleration_structure;
	const bvh_view bvh = make_bvh_view(structure);
	if (walk == ray_walk_binary) {
		k_closest_hits_binary<CULL_BACK><<<block_count(count, kBlock), kBlock, 0, stream>>>(bvh, rays, (uint32_t) count, out_hits);
		return hip_failed(hipGetLastError(), "trace_closest_hits");
	}
	const uint4* wide_nodes = (const uint4*) structure->wide_nodes;
	const uint32_t lds_entries = lds_option ? lds_option : kWideStackLds;
	return launch_wide("trace_closest_hits", structure, device, count, lds_entries, stream, [&](uint64_t first, uint64_t n, uint32_t* spill) {
		k_closest_hits_wide<CULL_BACK><<<block_count(n, kBlock), kBlock, 0, stream>>>(bvh, wide_nodes, rays + first, (uint32_t) n, out_hits + first, spill, lds_entries);
	});
}

extern "C" int trace_closest_hits(const scene_t* scene, const device_t* device, const ray_t* rays, uint64_t count, VkBool32 cull_back_faces, ray_hit_t* out_hits, const ray_query_options_t* options, void* stream) {
	uint32_t walk, lds_option;
	if (plan_query("trace_closest_hits", scene, device, count, options, &walk, &lds_option)) return 1;
	if (!count) return 0;
	hipStream_t s = (hipStream_t) (stream ? stream : device->stream);
	return cull_back_faces ? launch_closest_hits<true>(scene, device, walk, lds_option, rays, count, out_hits, s) : launch_closest_hits<false>(scene, device, walk, lds_option, rays, count, out_hits, s);
}

extern "C" int trace_any_hits(const scene_t* scene, const device_t* device, const ray_t* rays, uint64_t count, uint8_t* out_blocked, const ray_query_options_t* options, void* stream) {
	uint32_t walk, lds_option;
	if (plan_query("trace_any_hits", scene, device, count, options, &walk, &lds_option)) return 1;
	if (!count) return 0;
	hipStream_t s = (hipStream_t) (stream ? stream : device->stream);
	const acceleration_structure_t* structure = &scene->acceleration_structure;
	const bvh_view bvh = make_bvh_view(structure);
	if (walk == ray_walk_binary) {
		k_any_hits_binary<<<block_count(count, kBlock), kBlock, 0, s>>>(bvh, rays, (uint32_t) count, out_blocked);
		return hip_failed(hipGetLastError(), "trace_any_hits");
	}
	const uint4* wide_nodes = (const uint4*) structure->wide_nodes;
	const uint32_t lds_entries = lds_option ? lds_option : kWideStackLds;
	return launch_wide("trace_any_hits", structure, device, count, lds_entries, s, [&](uint64_t first, uint64_t n, uint32_t* spill) {
		k_any_hits_wide<<<block_count(n, kBlock), kBlock, 0, s>>>(bvh, wide_nodes, rays + first, (uint32_t) n, out_blocked + first, spill, lds_entries);
	});
}
