// Meshes exported to *.vks scenes on the device (include/vkr_scene_export.h export_scene): the boxes of the vertices and
// of the centroids by a reduction that also validates the inputs, one 16-byte record per vertex (packed position, normal
// codes), Morton keys sorted by hipcub, and one lane per output triangle that gathers its three records and packs its
// texture coordinates.  Compiled without contraction and with correctly rounded divisions like texture_conversion.hip;
// every buffer is restated in numpy byte for byte (vulkan_renderer_amd/scene_export.py).
#include "vkr_scene_export.h"
#include "host/vkr_internal.h"
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

constexpr uint32_t kBlock = 256, kWave = 64;
// the reductions run over at most this many workgroups (each ends in six atomics on the same words)
constexpr uint32_t kMostReductionBlocks = 1024;

enum : uint32_t { kFlagVertexIndex = 1u, kFlagMaterialIndex = 2u, kFlagNotFinite = 4u };

// What the kernels share in device memory: the boxes as order-preserving integer images of their floats, and the flags
struct export_state {
	uint32_t vertex_lo[3], vertex_hi[3], centroid_lo[3], centroid_hi[3];
	uint32_t flags;
};

struct export_args {
	// the source arrays on the device; indices, tex_coords and materials may be NULL (vkr_scene_export.h)
	const float* positions;
	const float* normals;
	const uint32_t* indices;
	const float* tex_coords;
	const uint8_t* materials;
	export_state* state;
	// 3 floats per triangle (only when sorting)
	float* centroids;
	// per vertex: the two position words, the normal codes (x in the low half), padding
	uint4* records;
	// (code << 32) | triangle, sorted; NULL: the input order
	const uint64_t* sorted_keys;
	uint64_t* keys;
	uint32_t* out_positions;
	uint16_t* out_normals_and_tex_coords;
	uint8_t* out_materials;
	uint64_t vertex_count;
	uint32_t triangle_count, material_count;
	// quantisation factor and offset of the vertex box, Morton factor and offset of the centroid box (made on the host)
	float qf[3], qo[3], mf[3], mo[3];
};

// ---- boxes and validation ----------------------------------------------------------------------------------------------

// Unsigned integers in the order of the floats (-0 below +0)
__device__ static inline uint32_t ordered_image(float value) {
	uint32_t u = __float_as_uint(value);
	return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

static float float_of_ordered_image(uint32_t image) {
	uint32_t u = (image & 0x80000000u) ? (image & 0x7FFFFFFFu) : ~image;
	float value;
	memcpy(&value, &u, sizeof(value));
	return value;
}

__device__ static inline bool is_finite(float value) { return (__float_as_uint(value) & 0x7F800000u) != 0x7F800000u; }

// Reduces lo / hi over the workgroup (wave by shuffles, waves through LDS) and merges them into the box by atomics on
// the ordered images: minima and maxima do not depend on the order, so the box is deterministic.  Lanes without an
// element bring +infinity / -infinity.
__device__ static inline void merge_box(float lo[3], float hi[3], uint32_t* box_lo, uint32_t* box_hi, uint32_t flags, uint32_t* box_flags) {
	__shared__ float partial[kBlock / kWave][6];
	__shared__ uint32_t partial_flags[kBlock / kWave];
	for (uint32_t offset = kWave / 2; offset != 0; offset >>= 1) {
#pragma unroll
		for (uint32_t j = 0; j != 3; ++j) {
			lo[j] = fminf(lo[j], __shfl_down(lo[j], offset, kWave));
			hi[j] = fmaxf(hi[j], __shfl_down(hi[j], offset, kWave));
		}
		flags |= (uint32_t) __shfl_down((int) flags, offset, kWave);
	}
	uint32_t wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
	if (lane == 0) {
		for (uint32_t j = 0; j != 3; ++j) { partial[wave][j] = lo[j]; partial[wave][3 + j] = hi[j]; }
		partial_flags[wave] = flags;
	}
	__syncthreads();
	if (threadIdx.x < 3) {
		uint32_t j = threadIdx.x;
		float l = partial[0][j], h = partial[0][3 + j];
		for (uint32_t w = 1; w != kBlock / kWave; ++w) { l = fminf(l, partial[w][j]); h = fmaxf(h, partial[w][3 + j]); }
		atomicMin(&box_lo[j], ordered_image(l));
		atomicMax(&box_hi[j], ordered_image(h));
	}
	if (threadIdx.x == 3) {
		uint32_t all = 0;
		for (uint32_t w = 0; w != kBlock / kWave; ++w) all |= partial_flags[w];
		if (all) atomicOr(box_flags, all);
	}
}

// fminf / fmaxf drop a NaN; -0 and +0 compare equal, so the one kept depends on the order: the host stores zeros as +0
__global__ void __launch_bounds__(kBlock) k_vertex_box(export_args a) {
	float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
	uint32_t flags = 0;
	for (uint64_t v = (uint64_t) blockIdx.x * kBlock + threadIdx.x; v < a.vertex_count; v += (uint64_t) gridDim.x * kBlock) {
#pragma unroll
		for (uint32_t j = 0; j != 3; ++j) {
			float p = a.positions[3 * v + j];
			if (!is_finite(p) || !is_finite(a.normals[3 * v + j])) flags |= kFlagNotFinite;
			lo[j] = fminf(lo[j], p);
			hi[j] = fmaxf(hi[j], p);
		}
	}
	merge_box(lo, hi, a.state->vertex_lo, a.state->vertex_hi, flags, &a.state->flags);
}

// The vertex indices of a triangle
__device__ static inline void triangle_vertices(uint32_t out[3], const export_args& a, uint32_t triangle) {
#pragma unroll
	for (uint32_t k = 0; k != 3; ++k) out[k] = a.indices ? a.indices[3 * (size_t) triangle + k] : (3 * triangle + k);
}

// Validates what belongs to a triangle - an index is compared with the vertex count before anything is read through it -
// and, when sorting, stores the centroid ((p0 + p1) + p2) / 3.0f and reduces the centroids' box
__global__ void __launch_bounds__(kBlock) k_triangle_box(export_args a) {
	float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
	uint32_t flags = 0;
	for (uint32_t t = blockIdx.x * kBlock + threadIdx.x; t < a.triangle_count; t += gridDim.x * kBlock) {
		uint32_t vertices[3];
		triangle_vertices(vertices, a, t);
		bool in_range = vertices[0] < a.vertex_count && vertices[1] < a.vertex_count && vertices[2] < a.vertex_count;
		if (!in_range) flags |= kFlagVertexIndex;
		if (a.materials && a.materials[t] >= a.material_count) flags |= kFlagMaterialIndex;
		if (a.tex_coords)
			for (uint32_t i = 0; i != 6; ++i)
				if (!is_finite(a.tex_coords[6 * (size_t) t + i])) flags |= kFlagNotFinite;
		if (a.centroids && in_range) {
#pragma unroll
			for (uint32_t j = 0; j != 3; ++j) {
				float c = ((a.positions[3 * (size_t) vertices[0] + j] + a.positions[3 * (size_t) vertices[1] + j]) + a.positions[3 * (size_t) vertices[2] + j]) / 3.0f;
				a.centroids[3 * (size_t) t + j] = c;
				lo[j] = fminf(lo[j], c);
				hi[j] = fmaxf(hi[j], c);
			}
		}
	}
	merge_box(lo, hi, a.state->centroid_lo, a.state->centroid_hi, flags, &a.state->flags);
}

// ---- records, keys, output ---------------------------------------------------------------------------------------------

// (uint16_t) trunc(o * 32767.0 + 32768.5) in binary64
__device__ static inline uint32_t normal_code(float o) { return (uint32_t) ((double) o * 32767.0 + 32768.5); }

// One lane per vertex
__global__ void __launch_bounds__(kBlock) k_vertex_records(export_args a) {
	uint64_t v = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
	if (v >= a.vertex_count) return;
	uint32_t q[3];
#pragma unroll
	for (uint32_t j = 0; j != 3; ++j) {
		uint32_t cell = (uint32_t) (a.positions[3 * v + j] * a.qf[j] + a.qo[j]);
		q[j] = cell < 0x1FFFFFu ? cell : 0x1FFFFFu;
	}
	float x = a.normals[3 * v], y = a.normals[3 * v + 1], z = a.normals[3 * v + 2];
	float l = (fabsf(x) + fabsf(y)) + fabsf(z);
	float ox = x / l, oy = y / l;
	if (z <= 0.0f) {
		float fx = (1.0f - fabsf(oy)) * (ox >= 0.0f ? 1.0f : -1.0f);
		float fy = (1.0f - fabsf(ox)) * (oy >= 0.0f ? 1.0f : -1.0f);
		ox = fx; oy = fy;
	}
	uint32_t nx = normal_code(ox), ny = normal_code(oy);
	if (l == 0.0f) nx = ny = 32768u;
	uint4 record;
	record.x = q[0] + ((q[1] & 0x7FFu) << 21);
	record.y = ((q[1] & 0x1FF800u) >> 11) + (q[2] << 10);
	record.z = (nx & 0xFFFFu) | (ny << 16);
	record.w = 0;
	a.records[v] = record;
}

// Two zero bits between any two of the low ten bits (reference tools/io_export_vulkan_blender28.py:49-63)
__device__ static inline uint32_t spread(uint32_t x) {
	x &= 0x000003FFu;
	x = (x ^ (x << 16)) & 0xFF0000FFu;
	x = (x ^ (x << 8)) & 0x0300F00Fu;
	x = (x ^ (x << 4)) & 0x030C30C3u;
	x = (x ^ (x << 2)) & 0x09249249u;
	return x;
}

// One lane per triangle: the low word of the key keeps triangles of equal code in input order
__global__ void __launch_bounds__(kBlock) k_morton_keys(export_args a) {
	uint32_t t = blockIdx.x * kBlock + threadIdx.x;
	if (t >= a.triangle_count) return;
	uint32_t g[3];
#pragma unroll
	for (uint32_t j = 0; j != 3; ++j)
		g[j] = (uint32_t) fminf(fmaxf(a.centroids[3 * (size_t) t + j] * a.mf[j] + a.mo[j], 0.0f), 1023.0f);
	uint32_t code = spread(g[0]) | (spread(g[1]) << 1) | (spread(g[2]) << 2);
	a.keys[t] = ((uint64_t) code << 32) | t;
}

// One lane per output triangle.  The 24 + 24 bytes of a triangle go through LDS, so that the lanes of a wave store
// consecutive 8-byte pieces of the workgroup's range instead of pieces 24 bytes apart.
__global__ void __launch_bounds__(kBlock) k_write_triangles(export_args a) {
	__shared__ uint32_t staged_positions[kBlock * 6];
	__shared__ uint32_t staged_codes[kBlock * 6];
	uint32_t first = blockIdx.x * kBlock, t = first + threadIdx.x;
	if (t < a.triangle_count) {
		uint32_t source = a.sorted_keys ? (uint32_t) a.sorted_keys[t] : t;
		uint32_t vertices[3];
		triangle_vertices(vertices, a, source);
		float uv[3][2] = {{0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}};
		if (a.tex_coords) {
#pragma unroll
			for (uint32_t i = 0; i != 6; ++i) uv[i / 2][i % 2] = a.tex_coords[6 * (size_t) source + i];
		}
		float shift[2];
#pragma unroll
		for (uint32_t i = 0; i != 2; ++i) shift[i] = floorf(fminf(fminf(uv[0][i], uv[1][i]), uv[2][i]));
#pragma unroll
		for (uint32_t k = 0; k != 3; ++k) {
			uint4 record = a.records[vertices[k]];
			uint32_t u = (uint32_t) fminf(fmaxf((uv[k][0] - shift[0]) * 8191.875f + 0.5f, 0.0f), 65535.0f);
			uint32_t v = (uint32_t) fminf(fmaxf((uv[k][1] - shift[1]) * 8191.875f + 0.5f, 0.0f), 65535.0f);
			staged_positions[threadIdx.x * 6 + 2 * k] = record.x;
			staged_positions[threadIdx.x * 6 + 2 * k + 1] = record.y;
			staged_codes[threadIdx.x * 6 + 2 * k] = record.z;
			staged_codes[threadIdx.x * 6 + 2 * k + 1] = u | (v << 16);
		}
		a.out_materials[t] = a.materials ? a.materials[source] : (uint8_t) 0;
	}
	__syncthreads();
	uint32_t count = a.triangle_count - first;
	count = count < kBlock ? count : kBlock;
	// (24 bytes per triangle: the workgroup's range starts at a multiple of 8 bytes)
	uint2* positions = (uint2*) (a.out_positions + (size_t) first * 6);
	uint2* codes = (uint2*) ((uint32_t*) a.out_normals_and_tex_coords + (size_t) first * 6);
	for (uint32_t i = threadIdx.x; i < count * 3; i += kBlock) {
		positions[i] = make_uint2(staged_positions[2 * i], staged_positions[2 * i + 1]);
		codes[i] = make_uint2(staged_codes[2 * i], staged_codes[2 * i + 1]);
	}
}

// ---- host ----------------------------------------------------------------------------------------------------------------

static inline uint32_t reduction_block_count(uint64_t lanes) {
	uint64_t blocks = (lanes + kBlock - 1) / kBlock;
	return (uint32_t) (blocks < kMostReductionBlocks ? blocks : kMostReductionBlocks);
}

static float last_kernel_milliseconds = 0.0f;
extern "C" float get_scene_export_kernel_milliseconds(void) { return last_kernel_milliseconds; }

extern "C" int export_scene(exported_scene_t* out, const device_t* device, const scene_export_source_t* source, VkBool32 sort_triangles) {
	memset(out, 0, sizeof(*out));
	if (!device) {
		printf("export_scene() needs a device: the exporter is HIP kernels.\n");
		return 1;
	}
	if (!source || source->triangle_count == 0 || source->triangle_count > 0x7FFFFFFFull / 3) {
		printf("A scene has 1 ... %llu triangles, not %llu.\n", 0x7FFFFFFFull / 3, source ? (unsigned long long) source->triangle_count : 0ull);
		return 1;
	}
	if (source->material_count < 1 || source->material_count > 256) {
		printf("A scene has 1 ... 256 materials, not %llu.\n", (unsigned long long) source->material_count);
		return 1;
	}
	int arrays_missing = !source->vertex_positions || !source->vertex_normals || !source->material_names;
	for (uint64_t i = 0; !arrays_missing && i != source->material_count; ++i) arrays_missing = !source->material_names[i];
	if (arrays_missing) {
		printf("export_scene() needs vertex positions, vertex normals and %llu material names.\n", (unsigned long long) source->material_count);
		return 1;
	}
	const uint64_t V = source->vertex_count;
	const uint32_t T = (uint32_t) source->triangle_count;
	// one device buffer for the source arrays, one for the temporaries, one for what is read back
	size_t attribute_bytes = sizeof(float) * 3 * V;
	size_t index_bytes = source->vertex_indices ? sizeof(uint32_t) * 3 * (size_t) T : 0, tex_coord_bytes = source->corner_tex_coords ? sizeof(float) * 6 * (size_t) T : 0;
	size_t material_bytes = source->material_indices ? (size_t) T : 0;
	size_t source_bytes = 0, temporary_bytes = 0, output_bytes = 0, sort_bytes = 0;
	if (sort_triangles && hipcub::DeviceRadixSort::SortKeys(NULL, sort_bytes, (const uint64_t*) NULL, (uint64_t*) NULL, (int) T, 0, 62, (hipStream_t) device->stream) != hipSuccess) {
		printf("Failed to size the sort of %u triangles.\n", T);
		return 1;
	}
	size_t position_bytes = sizeof(uint32_t) * 6 * (size_t) T, code_bytes = sizeof(uint16_t) * 12 * (size_t) T;
	// (the positions, the export_state and the packed positions are what the three buffers begin with)
	vkr_carve(&source_bytes, attribute_bytes);
	const size_t normals_at = vkr_carve(&source_bytes, attribute_bytes), indices_at = vkr_carve(&source_bytes, index_bytes);
	const size_t tex_coords_at = vkr_carve(&source_bytes, tex_coord_bytes), materials_at = vkr_carve(&source_bytes, material_bytes);
	vkr_carve(&temporary_bytes, sizeof(export_state));
	const size_t records_at = vkr_carve(&temporary_bytes, sizeof(uint4) * V), centroids_at = vkr_carve(&temporary_bytes, sort_triangles ? sizeof(float) * 3 * (size_t) T : 0);
	const size_t keys_at = vkr_carve(&temporary_bytes, sort_triangles ? sizeof(uint64_t) * T : 0), sorted_keys_at = vkr_carve(&temporary_bytes, sort_triangles ? sizeof(uint64_t) * T : 0);
	const size_t sort_storage_at = vkr_carve(&temporary_bytes, sort_bytes);
	vkr_carve(&output_bytes, position_bytes);
	const size_t codes_at = vkr_carve(&output_bytes, code_bytes), out_materials_at = vkr_carve(&output_bytes, T);

	out->triangle_count = T;
	out->positions = (uint32_t*) malloc(position_bytes);
	out->normals_and_tex_coords = (uint16_t*) malloc(code_bytes);
	out->material_indices = (uint8_t*) malloc(T);
	int failed = !out->positions || !out->normals_and_tex_coords || !out->material_indices || vkr_scene_export_copy_names(out, source);
	if (failed) printf("Out of memory for a scene of %u triangles.\n", T);
	void *source_device = NULL, *temporaries = NULL, *output = NULL;
	failed = failed || vkr_device_alloc(&source_device, device, source_bytes, "the source mesh") || vkr_device_alloc(&temporaries, device, temporary_bytes, "the vertex records and sort keys")
		|| vkr_device_alloc(&output, device, output_bytes, "the exported scene");
	hipStream_t stream = (hipStream_t) device->stream;
	hipEvent_t kernels_begin = NULL, kernels_end = NULL;
	failed = failed || hip_failed(hipEventCreate(&kernels_begin), "creating an event") || hip_failed(hipEventCreate(&kernels_end), "creating an event");

	export_args args;
	memset(&args, 0, sizeof(args));
	export_state initial_state;
	if (!failed) {
		uint8_t* base = (uint8_t*) source_device;
		args.positions = (const float*) base; args.normals = (const float*) (base + normals_at);
		args.indices = source->vertex_indices ? (const uint32_t*) (base + indices_at) : NULL;
		args.tex_coords = source->corner_tex_coords ? (const float*) (base + tex_coords_at) : NULL;
		args.materials = source->material_indices ? (const uint8_t*) (base + materials_at) : NULL;
		base = (uint8_t*) temporaries;
		args.state = (export_state*) base; args.records = (uint4*) (base + records_at);
		if (sort_triangles) { args.centroids = (float*) (base + centroids_at); args.keys = (uint64_t*) (base + keys_at); }
		base = (uint8_t*) output;
		args.out_positions = (uint32_t*) base; args.out_normals_and_tex_coords = (uint16_t*) (base + codes_at); args.out_materials = base + out_materials_at;
		args.vertex_count = V; args.triangle_count = T; args.material_count = (uint32_t) source->material_count;
		// (the images of +infinity and -infinity, and no flags)
		for (uint32_t j = 0; j != 3; ++j) {
			initial_state.vertex_lo[j] = initial_state.centroid_lo[j] = 0xFFFFFFFFu;
			initial_state.vertex_hi[j] = initial_state.centroid_hi[j] = 0u;
		}
		initial_state.flags = 0;
		failed = vkr_copy_to_device_async((void*) args.positions, source->vertex_positions, attribute_bytes, device)
			|| vkr_copy_to_device_async((void*) args.normals, source->vertex_normals, attribute_bytes, device)
			|| (args.indices && vkr_copy_to_device_async((void*) args.indices, source->vertex_indices, index_bytes, device))
			|| (args.tex_coords && vkr_copy_to_device_async((void*) args.tex_coords, source->corner_tex_coords, tex_coord_bytes, device))
			|| (args.materials && vkr_copy_to_device_async((void*) args.materials, source->material_indices, material_bytes, device))
			|| vkr_copy_to_device_async(args.state, &initial_state, sizeof(initial_state), device);
	}
	export_state state;
	if (!failed) {
		(void) hipEventRecord(kernels_begin, stream);
		if (V) k_vertex_box<<<reduction_block_count(V), kBlock, 0, stream>>>(args);
		k_triangle_box<<<reduction_block_count(T), kBlock, 0, stream>>>(args);
		// the boxes and the flags: nothing is read through an index before the flags have come back clear
		failed = hip_failed(hipGetLastError(), "reducing the boxes") || vkr_copy_to_host(&state, args.state, sizeof(state), device);
	}
	if (!failed && state.flags) {
		if (state.flags & kFlagVertexIndex) printf("The mesh has a vertex index that is not below its vertex count %llu.\n", (unsigned long long) V);
		else if (state.flags & kFlagMaterialIndex) printf("The mesh has a material index that is not below its material count %u.\n", args.material_count);
		else printf("The mesh has a position, normal or texture coordinate that is not finite.\n");
		failed = 1;
	}
	if (!failed) {
		float lo[3], hi[3];
		for (uint32_t j = 0; j != 3; ++j) { lo[j] = float_of_ordered_image(state.vertex_lo[j]); hi[j] = float_of_ordered_image(state.vertex_hi[j]); }
		vkr_scene_export_box_constants(args.qf, args.qo, lo, hi, 2097152.0f);
		vkr_scene_export_dequantization(out, args.qf, lo, hi);
		k_vertex_records<<<block_count(V, kBlock), kBlock, 0, stream>>>(args);
		failed = hip_failed(hipGetLastError(), "packing the vertices");
	}
	if (!failed && sort_triangles) {
		float lo[3], hi[3];
		for (uint32_t j = 0; j != 3; ++j) { lo[j] = float_of_ordered_image(state.centroid_lo[j]); hi[j] = float_of_ordered_image(state.centroid_hi[j]); }
		vkr_scene_export_box_constants(args.mf, args.mo, lo, hi, 1024.0f);
		uint64_t* sorted_keys = (uint64_t*) ((uint8_t*) temporaries + sorted_keys_at);
		k_morton_keys<<<block_count(T, kBlock), kBlock, 0, stream>>>(args);
		failed = hip_failed(hipGetLastError(), "making the Morton keys")
			|| hip_failed(hipcub::DeviceRadixSort::SortKeys((uint8_t*) temporaries + sort_storage_at, sort_bytes, (const uint64_t*) args.keys, sorted_keys, (int) T, 0, 62, stream), "sorting the triangles");
		args.sorted_keys = sorted_keys;
	}
	if (!failed) {
		k_write_triangles<<<block_count(T, kBlock), kBlock, 0, stream>>>(args);
		failed = hip_failed(hipGetLastError(), "writing the triangles");
		(void) hipEventRecord(kernels_end, stream);
	}
	if (!failed)
		failed = hip_failed(hipMemcpyAsync(out->positions, args.out_positions, position_bytes, hipMemcpyDeviceToHost, stream), "reading back")
			|| hip_failed(hipMemcpyAsync(out->normals_and_tex_coords, args.out_normals_and_tex_coords, code_bytes, hipMemcpyDeviceToHost, stream), "reading back")
			|| vkr_copy_to_host(out->material_indices, args.out_materials, T, device);
	// (the uploads and kernels that were queued read the source and the temporaries)
	else (void) hipStreamSynchronize(stream);
	if (!failed && hipEventElapsedTime(&last_kernel_milliseconds, kernels_begin, kernels_end) != hipSuccess) last_kernel_milliseconds = 0.0f;
	if (kernels_begin) (void) hipEventDestroy(kernels_begin);
	if (kernels_end) (void) hipEventDestroy(kernels_end);
	vkr_device_free(source_device, device); vkr_device_free(temporaries, device); vkr_device_free(output, device);
	if (failed) free_exported_scene(out);
	return failed;
}
