/* Host-only check of vkr_carve() (csrc/host/vkr_hip.h) as its users call it: the three arenas of csrc/bvh_build.hip and
 * the three buffers of csrc/scene_export.hip, sizes only, for meshes from one triangle to 2^31 / 16.  Every sub-range
 * must be 256-aligned, behind the one before it and inside the total, and the totals must be what the hand-written
 * offset sums gave before the helper existed (restated below as `expected`).  Needs no GPU:
 *   gcc -std=gnu99 -g -fsanitize=address,undefined -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Ivulkan_renderer_amd/csrc/host \
 *       profiles/tools/arena_layout_check.c -o /tmp/arena_layout_check && /tmp/arena_layout_check */
#include "vkr_hip.h"
#include <assert.h>

/* sizes of the structs the arenas hold (bvh_build.hip, lbvh.h, scene_export.hip) */
enum { kOpenNode = 96, kBin = 28, kBinsPerNode = 3 * 16, kWideItem = 12, kBuildNode = 32, kExportState = 52 };

static size_t aligned(size_t bytes) { return (bytes + 255) & ~(size_t) 255; }

/* carves `count` ranges of the given sizes and checks them; returns the total */
static size_t carve_all(const size_t* sizes, int count) {
	size_t total = 0, end_of_last = 0;
	for (int i = 0; i != count; ++i) {
		size_t at = vkr_carve(&total, sizes[i]);
		assert(at % 256 == 0 && total % 256 == 0);
		assert(at >= end_of_last && at + sizes[i] <= total);
		end_of_last = at + sizes[i];
	}
	return total;
}

int main(void) {
	const uint64_t counts[] = {1, 2, 3, 17, 131840, 0x7FFFFFFFu / 16u};
	/* what hipcub asks for is not known here: nothing, an odd size, a large one */
	const size_t storage[] = {0, 1, 767, (size_t) 1 << 28};
	for (size_t c = 0; c != sizeof(counts) / sizeof(counts[0]); ++c)
		for (size_t s = 0; s != sizeof(storage) / sizeof(storage[0]); ++s) {
			const size_t n = (size_t) counts[c], sort_bytes = storage[s];
			/* build_sah_on_device: open nodes twice, bins, triangle_node, counters */
			const size_t open_capacity = n / 2 + 1;
			const size_t sah[] = {kOpenNode * open_capacity, kOpenNode * open_capacity, (size_t) kBin * kBinsPerNode * open_capacity, 4 * n, 4 * 2};
			size_t expected = 2 * aligned(kOpenNode * open_capacity) + aligned((size_t) kBin * kBinsPerNode * open_capacity) + aligned(4 * n) + 256;
			assert(carve_all(sah, 5) == expected);
			/* collapse_to_wide: two work lists, counters */
			const size_t wide[] = {kWideItem * n, kWideItem * n, 4 * 3};
			expected = 2 * aligned(kWideItem * n) + 256;
			assert(carve_all(wide, 3) == expected);
			/* build_lbvh_on_device: nine allocations until now, each at least as aligned as here */
			const size_t inner = n > 1 ? n - 1 : 1;
			const size_t lbvh[] = {kBuildNode * inner, 8 * n, 8 * n, 4 * 3 * 2 * n, 4 * 3 * 2 * n, 4 * n, 4 * inner, sort_bytes};
			expected = 0;
			for (int i = 0; i != 8; ++i) expected += aligned(lbvh[i]);
			assert(carve_all(lbvh, 8) == expected);
			/* split_long_triangles: counts, their prefix sums, the scan's storage */
			const size_t split[] = {4 * n, 4 * n, sort_bytes};
			assert(carve_all(split, 3) == 2 * aligned(4 * n) + aligned(sort_bytes));
			/* export_scene: T triangles of V = 3 T or T / 2 + 3 vertices, with and without the optional arrays and the sort */
			for (int variant = 0; variant != 4; ++variant) {
				const size_t T = n, V = (variant & 1) ? 3 * T : T / 2 + 3, sorted = (size_t) (variant >> 1);
				const size_t attribute_bytes = 4 * 3 * V, index_bytes = (variant & 1) ? 0 : 4 * 3 * T, tex_coord_bytes = (variant & 1) ? 0 : 4 * 6 * T, material_bytes = (variant & 1) ? 0 : T;
				const size_t source[] = {attribute_bytes, attribute_bytes, index_bytes, tex_coord_bytes, material_bytes};
				size_t normals_at = aligned(attribute_bytes), indices_at = normals_at + aligned(attribute_bytes), tex_coords_at = indices_at + aligned(index_bytes);
				size_t materials_at = tex_coords_at + aligned(tex_coord_bytes), source_bytes = materials_at + aligned(material_bytes);
				assert(carve_all(source, 5) == source_bytes);
				const size_t temporaries[] = {kExportState, 16 * V, sorted ? 4 * 3 * T : 0, sorted ? 8 * T : 0, sorted ? 8 * T : 0, sorted ? sort_bytes : 0};
				size_t records_at = aligned(kExportState), centroids_at = records_at + aligned(16 * V);
				size_t keys_at = centroids_at + (sorted ? aligned(4 * 3 * T) : 0), sorted_keys_at = keys_at + (sorted ? aligned(8 * T) : 0);
				size_t sort_storage_at = sorted_keys_at + (sorted ? aligned(8 * T) : 0), temporary_bytes = sort_storage_at + aligned(sorted ? sort_bytes : 0);
				assert(carve_all(temporaries, 6) == temporary_bytes);
				const size_t output[] = {4 * 6 * T, 2 * 12 * T, T};
				size_t codes_at = aligned(4 * 6 * T), out_materials_at = codes_at + aligned(2 * 12 * T), output_bytes = out_materials_at + aligned(T);
				assert(carve_all(output, 3) == output_bytes);
			}
		}
	printf("arena layouts: all sub-ranges aligned, in order and inside their totals; totals as before\n");
	return 0;
}
