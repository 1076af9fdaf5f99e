/* Host part of the scene exporter (include/vkr_scene_export.h): the constants the kernels of csrc/scene_export.hip take
 * from the reduced boxes, the material names with the substitutions of reference
 * tools/io_export_vulkan_blender28.py:489-490, the container writer of :470-531 and free.  Compiled without contraction. */
#include "vkr_internal.h"
#include "vkr_scene_export.h"

void vkr_scene_export_box_constants(float factor[3], float offset[3], float lo[3], const float hi[3], float scale) {
	for (uint32_t j = 0; j != 3; ++j) {
		/* (a zero of lo is stored as +0) */
		lo[j] += 0.0f;
		int flat = hi[j] == lo[j];
		factor[j] = flat ? 0.0f : (scale / (hi[j] - lo[j]));
		offset[j] = flat ? 0.0f : (-lo[j] * factor[j]);
	}
}

void vkr_scene_export_dequantization(exported_scene_t* scene, const float quantization_factor[3], const float lo[3], const float hi[3]) {
	for (uint32_t j = 0; j != 3; ++j) {
		scene->dequantization_factor[j] = (hi[j] == lo[j]) ? 0.0f : (1.0f / quantization_factor[j]);
		scene->dequantization_summand[j] = lo[j] + 0.5f * scene->dequantization_factor[j] + 0.0f;
	}
}

static int is_digit(char c) { return c >= '0' && c <= '9'; }

/*! malloc'ed copy of the name without a trailing ".ddd" and without any ".DoubleSided" */
static char* substitute_material_name(const char* name) {
	static const char removed[] = ".DoubleSided";
	const size_t removed_length = sizeof(removed) - 1;
	size_t length = strlen(name);
	if (length >= 4 && name[length - 4] == '.' && is_digit(name[length - 3]) && is_digit(name[length - 2]) && is_digit(name[length - 1]))
		length -= 4;
	char* result = (char*) malloc(length + 1);
	if (!result) return NULL;
	size_t written = 0;
	for (size_t i = 0; i != length;) {
		if (length - i >= removed_length && memcmp(name + i, removed, removed_length) == 0) i += removed_length;
		else result[written++] = name[i++];
	}
	result[written] = 0;
	return result;
}

int vkr_scene_export_copy_names(exported_scene_t* scene, const scene_export_source_t* source) {
	scene->material_names = (char**) calloc(source->material_count, sizeof(char*));
	if (!scene->material_names) return 1;
	scene->material_count = source->material_count;
	for (uint64_t i = 0; i != source->material_count; ++i)
		if (!(scene->material_names[i] = substitute_material_name(source->material_names[i]))) return 1;
	return 0;
}

VKR_API int write_exported_scene(const exported_scene_t* scene, const char* file_path) {
	if (!scene || !scene->positions || !scene->normals_and_tex_coords || !scene->material_indices || !scene->material_names) {
		printf("There is no exported scene to write to %s.\n", file_path ? file_path : "(null)");
		return 1;
	}
	FILE* file = file_path ? fopen(file_path, "wb") : NULL;
	if (!file) {
		printf("Failed to open the output file: %s\n", file_path ? file_path : "(null)");
		return 1;
	}
	uint32_t marker_version[2] = {0x00abcabc, 1}, eof_marker = 0x00e0fe0f;
	uint64_t counts[2] = {scene->material_count, scene->triangle_count};
	int failed = fwrite(marker_version, sizeof(uint32_t), 2, file) != 2 || fwrite(counts, sizeof(uint64_t), 2, file) != 2
		|| fwrite(scene->dequantization_factor, sizeof(float), 3, file) != 3 || fwrite(scene->dequantization_summand, sizeof(float), 3, file) != 3;
	for (uint64_t i = 0; i != scene->material_count && !failed; ++i) {
		uint64_t length = strlen(scene->material_names[i]);
		failed = fwrite(&length, sizeof(length), 1, file) != 1 || fwrite(scene->material_names[i], 1, length + 1, file) != length + 1;
	}
	size_t corner_count = (size_t) scene->triangle_count * 3;
	failed = failed || fwrite(scene->positions, sizeof(uint32_t) * 2, corner_count, file) != corner_count
		|| fwrite(scene->normals_and_tex_coords, sizeof(uint16_t) * 4, corner_count, file) != corner_count
		|| fwrite(scene->material_indices, 1, scene->triangle_count, file) != scene->triangle_count
		|| fwrite(&eof_marker, sizeof(eof_marker), 1, file) != 1;
	failed |= fclose(file) != 0;
	if (failed) printf("Failed to write the scene file at path %s.\n", file_path);
	return failed;
}

VKR_API void free_exported_scene(exported_scene_t* scene) {
	if (scene->material_names)
		for (uint64_t i = 0; i != scene->material_count; ++i) free(scene->material_names[i]);
	free(scene->material_names);
	free(scene->positions);
	free(scene->normals_and_tex_coords);
	free(scene->material_indices);
	memset(scene, 0, sizeof(*scene));
}
