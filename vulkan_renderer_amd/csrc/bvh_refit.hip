// Moving geometry (include/vkr_scene_update.h): new vertex positions for a loaded mesh, and a refit of the two traversal
// layouts of lbvh.h that keeps their topology and recomputes every box.  No reference counterpart: the reference builds
// its acceleration structure once (src/scene.c:142-406).
//
// A refit is five steps on device->stream with one host synchronisation in the middle:
//   1. k_refit_leaves    one lane per leaf slot: de-quantises the moved triangle, rewrites its record in triangle_vertices,
//                        computes the fp32 box of the leaf (of slab j of count of the triangle where the build has split
//                        it) and reduces the box of the mesh
//   2. the host reads that box and chooses the grid of the quantised boxes from it, exactly as the build does from its
//      root box: a refit and a fresh build of the same mesh share one grid
//   3. k_refit_binary    one lane per leaf slot quantises its box and climbs the binary tree
//   4. k_refit_wide      one lane per four-wide node fills the lanes that name leaves and climbs the wide tree
//   5. k_tree_cost       (when asked) the half-areas of the inner binary nodes, as three exact integer sums
// Everything behind the leaf boxes is a minimum or a maximum of 15-bit integers, hence exact and independent of any order.
// Quantisation is monotone per coordinate - the floor of the minimum is the minimum of the floors - so the inner boxes
// are computed from the packed boxes of the children, and a refit of unmoved vertices gives the bytes of the build.
//
// The bottom-up passes (3 and 4) are last-arriver climbs: every inner node has a counter, a lane that has written a box
// adds one to the counter of the parent, and the lane whose addition completes the count computes the parent's box from
// its children's and goes on; every other lane returns.  No lane ever waits for another.  How a box written by one
// workgroup becomes visible to the last arriver in another (the L2s of the eight XCDs are not coherent with each other, a
// CU's L1 is never refreshed by another CU's stores) is `hand_off` below; DESIGN.md 4.15 has the measurements.
#include "vkr_scene_update.h"
#include "bvh_leaf_boxes.h"
#include "host/vkr_internal.h"
#include <hip/hip_runtime.h>

using namespace vkr;

namespace {

constexpr uint32_t kNoParent = 0xFFFFFFFFu;

// What the first update derives from the tree and every update uses.  Lives on the host (acceleration_structure_t.refit_state);
// the arrays are parts of one device allocation.
struct refit_state {
	void* arena;
	// what every update zeroes in front of its kernels, one block at the start of the arena: the box of the mesh (six words),
	// the sums of the cost (three uint64_t) and the arrival counters of the binary and of the wide nodes
	uint32_t* box_words;
	unsigned long long* cost_sums;
	uint32_t *binary_arrivals, *wide_arrivals;
	size_t zeroed_bytes;
	// parent of every binary node, binary node of every leaf slot
	uint32_t *binary_parent, *leaf_node;
	// wide node << 2 | lane that names every wide node, and how many lanes of a wide node name inner nodes
	uint32_t *wide_parent, *wide_inner;
	// lo.xyz, hi.xyz of every leaf slot, unpadded
	float* leaf_boxes;
	// pinned: where the host reads the box of the mesh and the sums
	uint32_t* host_words;
};

struct refit_mesh {
	const uint2* quantized_positions;
	float factor[3], summand[3];
};

// ---- the hand-off between workgroups -----------------------------------------------------------
// Boxes are stored and loaded with relaxed agent-scope atomics of 4 and 8 bytes: stores that are written through to memory
// (sc1) and loads that bypass the L1.  Between its stores and its addition to the counter a lane drains its stores
// (s_waitcnt vmcnt(0)): once the addition is performed, behind the L2s, the bytes are in memory - no release fence, which
// would write back the whole L2.  The lane whose addition completes the count, and no other, runs an agent-scope acquire
// (buffer_inv sc1) before it loads the children's boxes.  Links, parents and counts are not written by these launches and
// are loaded plainly.  (Measured against a fence on either side of the addition, and against no acquire at all: DESIGN.md
// 4.15.)
__device__ __forceinline__ void store_word(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t load_word(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void store_pair(void* p, uint32_t lo, uint32_t hi) { __hip_atomic_store((unsigned long long*) p, (unsigned long long) lo | ((unsigned long long) hi << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint2 load_pair(const void* p) {
	unsigned long long v = __hip_atomic_load((const unsigned long long*) p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	return make_uint2((uint32_t) v, (uint32_t) (v >> 32));
}
// true for the lane whose arrival is number `last` (counted from 0) at the counter
__device__ __forceinline__ bool arrive(uint32_t* counter, uint32_t last) {
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	const bool won = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == last;
	if (won) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
	return won;
}

// box of a binary node: x | y as one 8-byte word, z; the link behind them stays
__device__ __forceinline__ void store_box(uint4* node, uint32_t x, uint32_t y, uint32_t z) {
	store_pair(node, x, y);
	store_word((uint32_t*) node + 2, z);
}
__device__ __forceinline__ void load_box(const uint4* node, uint32_t (&q)[3]) {
	uint2 xy = load_pair(node);
	q[0] = xy.x; q[1] = xy.y; q[2] = load_word((const uint32_t*) node + 2);
}

// Union of two packed boxes (lo | hi << 16): packed 16-bit minimum and maximum, the low half of the one and the high half of the other
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t merge_packed(uint32_t a, uint32_t b) {
	u16x2 va = __builtin_bit_cast(u16x2, a), vb = __builtin_bit_cast(u16x2, b);
	uint32_t least = __builtin_bit_cast(uint32_t, __builtin_elementwise_min(va, vb)), most = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(va, vb));
	return (least & 0x0000FFFFu) | (most & 0xFFFF0000u);
}

// ---- what the first update derives ----------------------------------------------------------------

// The left child of an inner node is the next node; the right child is the left child's link, or two nodes on behind a leaf
__device__ __forceinline__ uint32_t right_child(const uint4* nodes, uint32_t node) {
	uint32_t left_link = nodes[node + 1u].w;
	return (left_link & kLeafBit) ? node + 2u : left_link;
}

__global__ void __launch_bounds__(256) k_derive_binary(const uint4* nodes, uint32_t node_count, uint32_t* binary_parent, uint32_t* leaf_node) {
	uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= node_count) return;
	if (i == 0u) binary_parent[0] = kNoParent;
	uint32_t link = nodes[i].w;
	if (link & kLeafBit) leaf_node[link & ~kLeafBit] = i;
	else {
		binary_parent[i + 1u] = i;
		binary_parent[right_child(nodes, i)] = i;
	}
}

__global__ void __launch_bounds__(256) k_derive_wide(const uint4* wide, uint32_t wide_node_count, uint32_t* wide_parent, uint32_t* wide_inner) {
	uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= wide_node_count) return;
	if (i == 0u) wide_parent[0] = kNoParent;
	uint4 links = wide[4 * (size_t) i + 3];
	const uint32_t link[4] = {links.x, links.y, links.z, links.w};
	uint32_t inner = 0;
	for (uint32_t c = 0; c != 4u; ++c)
		if (link[c] != kWideEmpty && !(link[c] & kLeafBit)) {
			wide_parent[link[c]] = (i << 2) | c;
			++inner;
		}
	wide_inner[i] = inner;
}

// ---- step 1 -----------------------------------------------------------------------------------------

// box_words: ~ordered(lo.xyz), ordered(hi.xyz), grown by atomicMax from zero
__global__ void __launch_bounds__(256) k_refit_leaves(refit_mesh mesh, uint32_t leaf_count, const uint32_t* leaf_fragments, float4* triangles, float* leaf_boxes, uint32_t* box_words) {
	__shared__ float wave_boxes[4][6];
	const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
	float box[6] = {3.0e38f, 3.0e38f, 3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f};
	if (slot < leaf_count) {
		float4* record = triangles + 3 * (size_t) slot;
		const float primitive = record[0].w;
		const uint32_t triangle = __float_as_uint(primitive);
		f3 v[3];
		for (int i = 0; i != 3; ++i) v[i] = dequantize_position(mesh.quantized_positions[3 * (size_t) triangle + i], mesh.factor, mesh.summand);
		record[0] = make_float4(v[0].x, v[0].y, v[0].z, primitive);
		record[1] = make_float4(v[1].x, v[1].y, v[1].z, 0.0f);
		record[2] = make_float4(v[2].x, v[2].y, v[2].z, 0.0f);
		f3 lo = mk3(fminf(v[0].x, fminf(v[1].x, v[2].x)), fminf(v[0].y, fminf(v[1].y, v[2].y)), fminf(v[0].z, fminf(v[1].z, v[2].z)));
		f3 hi = mk3(fmaxf(v[0].x, fmaxf(v[1].x, v[2].x)), fmaxf(v[0].y, fmaxf(v[1].y, v[2].y)), fmaxf(v[0].z, fmaxf(v[1].z, v[2].z)));
		const uint32_t fragment = leaf_fragments[slot], count = fragment & 0xFFFFu;
		if (count > 1u) {
			f3 flo, fhi;
			fragment_bounds(v, lo, hi, longest_axis(lo, hi), fragment >> 16, count, flo, fhi);
			lo = flo; hi = fhi;
		}
		box[0] = lo.x; box[1] = lo.y; box[2] = lo.z; box[3] = hi.x; box[4] = hi.y; box[5] = hi.z;
		for (int j = 0; j != 6; ++j) leaf_boxes[6 * (size_t) slot + j] = box[j];
	}
	// the box of the mesh: across the wave, across the waves of the workgroup through LDS, six atomics per workgroup
	for (int offset = 32; offset > 0; offset >>= 1)
		for (int j = 0; j != 3; ++j) {
			box[j] = fminf(box[j], __shfl_xor(box[j], offset));
			box[3 + j] = fmaxf(box[3 + j], __shfl_xor(box[3 + j], offset));
		}
	if ((threadIdx.x & 63u) == 0u)
		for (int j = 0; j != 6; ++j) wave_boxes[threadIdx.x >> 6][j] = box[j];
	__syncthreads();
	if (threadIdx.x < 6u) {
		const uint32_t j = threadIdx.x;
		float a = wave_boxes[0][j];
		for (int wave = 1; wave != 4; ++wave) a = j < 3u ? fminf(a, wave_boxes[wave][j]) : fmaxf(a, wave_boxes[wave][j]);
		atomicMax(&box_words[j], j < 3u ? ~ordered(a) : ordered(a));
	}
}

// ---- step 3 -----------------------------------------------------------------------------------------

struct refit_grid {
	float origin[3], inverse_cell[3], pad;
};

__global__ void __launch_bounds__(256) k_refit_binary(uint32_t leaf_count, const float* leaf_boxes, refit_grid grid, uint4* nodes, const uint32_t* leaf_node, const uint32_t* binary_parent, uint32_t* arrivals) {
	const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
	if (slot >= leaf_count) return;
	const float* box = leaf_boxes + 6 * (size_t) slot;
	uint32_t q[3];
	// (padded like write_threaded_node / k_write_leaves / sah_bvh.c write_node, quantised like k_quantize_nodes)
	for (int j = 0; j != 3; ++j) q[j] = quantize_box_axis(box[j] - grid.pad, box[3 + j] + grid.pad, grid.origin[j], grid.inverse_cell[j]);
	uint32_t node = leaf_node[slot];
	store_box(nodes + node, q[0], q[1], q[2]);
	for (node = binary_parent[node]; node != kNoParent; node = binary_parent[node]) {
		// the second of the two children to arrive goes on
		if (!arrive(&arrivals[node], 1u)) return;
		uint32_t a[3], b[3];
		load_box(nodes + node + 1u, a);
		load_box(nodes + right_child(nodes, node), b);
		store_box(nodes + node, merge_packed(a[0], b[0]), merge_packed(a[1], b[1]), merge_packed(a[2], b[2]));
	}
}

// ---- step 4 -----------------------------------------------------------------------------------------

// Refits the wide tree on its own from the quantised leaf boxes that step 3 has left in the binary nodes (a launch
// earlier, hence visible).  A wide node is complete when its own lane has filled the lanes that name leaves and every
// inner child has written its union into the lane that names it: wide_inner + 1 arrivals.  The node's own lane counting
// as one is what keeps a child that finishes early from publishing a node whose leaf lanes are not written yet.
__global__ void __launch_bounds__(256) k_refit_wide(uint32_t wide_node_count, uint4* wide, const uint4* nodes, const uint32_t* leaf_node, const uint32_t* wide_parent, const uint32_t* wide_inner, uint32_t* arrivals) {
	uint32_t node = blockIdx.x * blockDim.x + threadIdx.x;
	if (node >= wide_node_count) return;
	{
		uint32_t* words = (uint32_t*) (wide + 4 * (size_t) node);
		const uint4 links = wide[4 * (size_t) node + 3];
		const uint32_t link[4] = {links.x, links.y, links.z, links.w};
		for (uint32_t c = 0; c != 4u; ++c)
			if (link[c] != kWideEmpty && (link[c] & kLeafBit)) {
				const uint4 leaf = nodes[leaf_node[link[c] & ~kLeafBit]];
				store_word(words + c, leaf.x); store_word(words + 4 + c, leaf.y); store_word(words + 8 + c, leaf.z);
			}
	}
	for (;;) {
		if (!arrive(&arrivals[node], wide_inner[node])) return;
		const uint32_t parent = wide_parent[node];
		if (parent == kNoParent) return;
		const uint4* own = wide + 4 * (size_t) node;
		const uint4 links = own[3];
		const uint32_t link[4] = {links.x, links.y, links.z, links.w};
		// (an absent lane holds kWideEmptyBox, lo > hi, which must not take part)
		uint32_t merged[3] = {0, 0, 0};
		bool first = true;
		for (int axis = 0; axis != 3; ++axis) {
			const uint2 lanes01 = load_pair(own + axis), lanes23 = load_pair((const uint32_t*) (own + axis) + 2);
			const uint32_t q[4] = {lanes01.x, lanes01.y, lanes23.x, lanes23.y};
			first = true;
			for (uint32_t c = 0; c != 4u; ++c)
				if (link[c] != kWideEmpty) {
					merged[axis] = first ? q[c] : merge_packed(merged[axis], q[c]);
					first = false;
				}
		}
		uint32_t* words = (uint32_t*) (wide + 4 * (size_t) (parent >> 2)) + (parent & 3u);
		store_word(words, merged[0]); store_word(words + 4, merged[1]); store_word(words + 8, merged[2]);
		node = parent >> 2;
	}
}

// ---- step 5 -----------------------------------------------------------------------------------------

// sums[0 ... 2]: the sums of ex ey, ey ez, ez ex over the inner nodes, extents in cells
__global__ void __launch_bounds__(256) k_tree_cost(const uint4* nodes, uint32_t node_count, unsigned long long* sums) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	unsigned long long products[3] = {0ull, 0ull, 0ull};
	if (i < node_count) {
		const uint4 n = nodes[i];
		if (!(n.w & kLeafBit)) {
			const unsigned long long x = (n.x >> 16) - (n.x & 0xFFFFu), y = (n.y >> 16) - (n.y & 0xFFFFu), z = (n.z >> 16) - (n.z & 0xFFFFu);
			products[0] = x * y; products[1] = y * z; products[2] = z * x;
		}
	}
	for (int offset = 32; offset > 0; offset >>= 1)
		for (int j = 0; j != 3; ++j) products[j] += __shfl_xor(products[j], offset);
	if ((threadIdx.x & 63u) == 0u)
		for (int j = 0; j != 3; ++j)
			if (products[j]) atomicAdd(&sums[j], products[j]);
}

}  // namespace

// ---- host ---------------------------------------------------------------------------------------

extern "C" void vkr_free_refit_state(acceleration_structure_t* structure, const device_t* device) {
	refit_state* state = (refit_state*) structure->refit_state;
	if (!state) return;
	vkr_device_free(state->arena, device);
	vkr_host_free_pinned(state->host_words);
	free(state);
	structure->refit_state = NULL;
}

// The cost of include/vkr_scene_update.h from the three sums and the grid
static double scale_cost(const acceleration_structure_t* structure, const unsigned long long sums[3]) {
	double cell[3];
	for (int j = 0; j != 3; ++j) cell[j] = 1.0 / (double) structure->grid_inverse_cell[j];
	return (double) sums[0] * (cell[0] * cell[1]) + (double) sums[1] * (cell[1] * cell[2]) + (double) sums[2] * (cell[2] * cell[0]);
}

// Queues the cost kernel over the tree as it is and waits for its sums
static int measure_cost(const acceleration_structure_t* structure, refit_state* state, hipStream_t stream, double* out_cost) {
	unsigned long long* host_sums = (unsigned long long*) (state->host_words + 8);
	int failed = hip_failed(hipMemsetAsync(state->cost_sums, 0, 3 * sizeof(unsigned long long), stream), "clearing the sums of the tree cost");
	if (!failed) {
		k_tree_cost<<<block_count(structure->node_count, 256), 256, 0, stream>>>((const uint4*) structure->nodes, structure->node_count, state->cost_sums);
		failed = hip_failed(hipMemcpyAsync(host_sums, state->cost_sums, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream), "reading the sums of the tree cost")
			|| hip_failed(hipStreamSynchronize(stream), "measuring the cost of the tree");
	}
	if (!failed) *out_cost = scale_cost(structure, host_sums);
	return failed;
}

// The side arrays of the first update, and the cost of the tree as built
static int create_refit_state(acceleration_structure_t* structure, const device_t* device) {
	hipStream_t stream = (hipStream_t) device->stream;
	const uint32_t node_count = structure->node_count, leaf_count = structure->leaf_count, wide_count = structure->wide_nodes ? structure->wide_node_count : 0u;
	// (a wide parent is stored as node << 2 | lane)
	if (wide_count > 0x3FFFFFFFu) {
		printf("A four-wide tree of %u nodes is more than a refit supports (2^30 - 1).\n", wide_count);
		return 1;
	}
	refit_state* state = (refit_state*) calloc(1, sizeof(refit_state));
	if (!state) return 1;
	structure->refit_state = state;
	size_t arena_bytes = 0;
	// the zeroed block first (its size a multiple of 256, vkr_carve): box words, padding, sums, then the counters
	const size_t zeroed_at = vkr_carve(&arena_bytes, 64 + sizeof(uint32_t) * ((size_t) node_count + wide_count));
	state->zeroed_bytes = arena_bytes;
	const size_t binary_parent_at = vkr_carve(&arena_bytes, sizeof(uint32_t) * (size_t) node_count), leaf_node_at = vkr_carve(&arena_bytes, sizeof(uint32_t) * (size_t) leaf_count);
	const size_t wide_parent_at = vkr_carve(&arena_bytes, sizeof(uint32_t) * (size_t) wide_count), wide_inner_at = vkr_carve(&arena_bytes, sizeof(uint32_t) * (size_t) wide_count);
	const size_t leaf_boxes_at = vkr_carve(&arena_bytes, sizeof(float) * 6 * (size_t) leaf_count);
	int failed = vkr_device_alloc(&state->arena, device, arena_bytes, "the side arrays of the BVH refit") || vkr_host_alloc_pinned((void**) &state->host_words, 64);
	if (!failed) {
		uint8_t* base = (uint8_t*) state->arena;
		state->box_words = (uint32_t*) (base + zeroed_at);
		state->cost_sums = (unsigned long long*) (base + zeroed_at + 32);
		state->binary_arrivals = (uint32_t*) (base + zeroed_at + 64);
		state->wide_arrivals = state->binary_arrivals + node_count;
		state->binary_parent = (uint32_t*) (base + binary_parent_at); state->leaf_node = (uint32_t*) (base + leaf_node_at);
		state->wide_parent = (uint32_t*) (base + wide_parent_at); state->wide_inner = (uint32_t*) (base + wide_inner_at);
		state->leaf_boxes = (float*) (base + leaf_boxes_at);
		k_derive_binary<<<block_count(node_count, 256), 256, 0, stream>>>((const uint4*) structure->nodes, node_count, state->binary_parent, state->leaf_node);
		if (wide_count) k_derive_wide<<<block_count(wide_count, 256), 256, 0, stream>>>((const uint4*) structure->wide_nodes, wide_count, state->wide_parent, state->wide_inner);
		failed = hip_failed(hipGetLastError(), "deriving the side arrays of the BVH refit") || measure_cost(structure, state, stream, &structure->built_cost);
	}
	if (failed) vkr_free_refit_state(structure, device);
	return failed;
}

// Steps 1 to 4 (and 5 if out_cost is not NULL) for the positions that mesh->positions holds
static int refit(acceleration_structure_t* structure, const device_t* device, const mesh_t* mesh, double* out_cost) {
	hipStream_t stream = (hipStream_t) device->stream;
	if (!structure->refit_state && create_refit_state(structure, device)) return 1;
	refit_state* state = (refit_state*) structure->refit_state;
	const uint32_t leaf_count = structure->leaf_count, wide_count = structure->wide_nodes ? structure->wide_node_count : 0u;
	refit_mesh positions;
	positions.quantized_positions = (const uint2*) mesh->positions;
	for (int j = 0; j != 3; ++j) { positions.factor[j] = mesh->dequantization_factor[j]; positions.summand[j] = mesh->dequantization_summand[j]; }
	if (hip_failed(hipMemsetAsync(state->arena, 0, state->zeroed_bytes, stream), "clearing the counters of the BVH refit")) return 1;
	k_refit_leaves<<<block_count(leaf_count, 256), 256, 0, stream>>>(positions, leaf_count, (const uint32_t*) structure->leaf_fragments, (float4*) structure->triangle_vertices, state->leaf_boxes, state->box_words);
	// the update's one host synchronisation: the grid depends on the box of the moved mesh
	if (hip_failed(hipMemcpyAsync(state->host_words, state->box_words, 6 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream), "reading the box of the moved mesh")
		|| hip_failed(hipStreamSynchronize(stream), "computing the leaf boxes of the moved mesh")) return 1;
	refit_grid grid;
	grid.pad = vkr_bvh_padding(mesh);
	float lo[3], hi[3];
	for (int j = 0; j != 3; ++j) {
		// (the inverse of ordered() of bvh_leaf_boxes.h; padded like the root node of a build)
		const uint32_t l = ~state->host_words[j], h = state->host_words[3 + j];
		const uint32_t l_bits = (l & 0x80000000u) ? (l & 0x7FFFFFFFu) : ~l, h_bits = (h & 0x80000000u) ? (h & 0x7FFFFFFFu) : ~h;
		memcpy(&lo[j], &l_bits, sizeof(float)); memcpy(&hi[j], &h_bits, sizeof(float));
		lo[j] -= grid.pad; hi[j] += grid.pad;
	}
	vkr_choose_bvh_grid(structure, lo, hi);
	for (int j = 0; j != 3; ++j) { grid.origin[j] = structure->grid_origin[j]; grid.inverse_cell[j] = structure->grid_inverse_cell[j]; }
	k_refit_binary<<<block_count(leaf_count, 256), 256, 0, stream>>>(leaf_count, state->leaf_boxes, grid, (uint4*) structure->nodes, state->leaf_node, state->binary_parent, state->binary_arrivals);
	if (wide_count)
		k_refit_wide<<<block_count(wide_count, 256), 256, 0, stream>>>(wide_count, (uint4*) structure->wide_nodes, (const uint4*) structure->nodes, state->leaf_node, state->wide_parent, state->wide_inner, state->wide_arrivals);
	if (hip_failed(hipGetLastError(), "launching the kernels of the BVH refit")) return 1;
	if (out_cost) return measure_cost(structure, state, stream, out_cost);
	return hip_failed(hipStreamSynchronize(stream), "refitting the BVH");
}

// New contents for a device array of the mesh and, if asked, for its host copy
static int replace_mesh_array(void* device_array, void* host_copy, const void* source, size_t size, int source_on_device, int refresh_host_copy, const device_t* device, const char* what) {
	hipStream_t stream = (hipStream_t) device->stream;
	if (hip_failed(hipMemcpyAsync(device_array, source, size, source_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream), what)) return 1;
	if (!refresh_host_copy || !host_copy) return 0;
	if (!source_on_device) {
		memcpy(host_copy, source, size);
		return 0;
	}
	return hip_failed(hipMemcpyAsync(host_copy, source, size, hipMemcpyDeviceToHost, stream), what) || hip_failed(hipStreamSynchronize(stream), what);
}

VKR_API int update_scene_geometry(scene_t* scene, const device_t* device, const uint32_t* positions, const uint16_t* normals_and_tex_coords, const scene_update_options_t* options, scene_update_report_t* out_report) {
	scene_update_options_t o = {scene_update_refit, VK_FALSE, VK_TRUE, VK_FALSE, 0.0f};
	if (options) o = *options;
	if (!scene || !device || !positions) {
		printf("update_scene_geometry() needs a scene, a device and positions.\n");
		return 1;
	}
	if (o.policy > (uint32_t) scene_update_auto) {
		printf("Invalid scene update policy %u.\n", o.policy);
		return 1;
	}
	if (!(o.rebuild_above >= 0.0f)) {
		printf("scene_update_options_t.rebuild_above must not be negative or NaN, it is %g.\n", (double) o.rebuild_above);
		return 1;
	}
	mesh_t* mesh = &scene->mesh;
	acceleration_structure_t* structure = &scene->acceleration_structure;
	hipStream_t stream = (hipStream_t) device->stream;
	scene_update_report_t report;
	memset(&report, 0, sizeof(report));
	// frames of other streams may still read what is about to be written
	if (hip_failed(hipDeviceSynchronize(), "waiting for the device in front of a scene update")) return 1;
	hipEvent_t start = NULL, stop = NULL;
	int failed = hip_failed(hipEventCreate(&start), "creating an event") || hip_failed(hipEventCreate(&stop), "creating an event")
		|| hip_failed(hipEventRecord(start, stream), "recording the start of a scene update");
	const size_t vertex_count = 3 * (size_t) mesh->triangle_count;
	int host_positions_current = o.refresh_host_copy != VK_FALSE;
	failed = failed || replace_mesh_array(mesh->positions, mesh->host_positions, positions, sizeof(uint32_t) * 2 * vertex_count, o.inputs_on_device != VK_FALSE, o.refresh_host_copy != VK_FALSE, device, "replacing the vertex positions")
		|| (normals_and_tex_coords && replace_mesh_array(mesh->normals_and_tex_coords, mesh->host_normals_and_tex_coords, normals_and_tex_coords, sizeof(uint16_t) * 4 * vertex_count, o.inputs_on_device != VK_FALSE, o.refresh_host_copy != VK_FALSE, device, "replacing the normals and texture coordinates"));
	if (!failed && structure->nodes) {
		int rebuild = o.policy == (uint32_t) scene_update_rebuild;
		if (!rebuild) {
			const int want_cost = o.measure_cost != VK_FALSE || o.policy == (uint32_t) scene_update_auto;
			double cost = 0.0;
			failed = refit(structure, device, mesh, want_cost ? &cost : NULL);
			if (!failed) {
				structure->build_serial = vkr_next_build_serial();
				if (want_cost) { report.cost = cost; report.built_cost = structure->built_cost; }
				rebuild = o.policy == (uint32_t) scene_update_auto && o.rebuild_above > 0.0f && cost > (double) o.rebuild_above * structure->built_cost;
			}
		}
		if (!failed && rebuild) {
			const int builder = (int) structure->builder;
			// (the host builder reads the host copy)
			if (builder == (int) acceleration_structure_sah_host && !host_positions_current && mesh->host_positions)
				failed = vkr_copy_to_host(mesh->host_positions, mesh->positions, sizeof(uint32_t) * 2 * vertex_count, device);
			if (!failed) {
				vkr_destroy_acceleration_structure(structure, device);
				failed = vkr_build_acceleration_structure(structure, device, mesh, builder);
				report.rebuilt = 1u;
			}
		}
	}
	failed = failed || hip_failed(hipEventRecord(stop, stream), "recording the end of a scene update") || hip_failed(hipEventSynchronize(stop), "waiting for a scene update")
		|| hip_failed(hipEventElapsedTime(&report.milliseconds, start, stop), "timing a scene update");
	if (start) (void) hipEventDestroy(start);
	if (stop) (void) hipEventDestroy(stop);
	report.build_serial = structure->build_serial;
	if (out_report) *out_report = report;
	return failed;
}
