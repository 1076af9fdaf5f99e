/* Host part of the texture converter (include/vkr_texture_conversion.h): the container writer of reference
 * tools/texture_conversion/main.c:271-291, 398-399 and what the kernels of csrc/texture_conversion.hip take from the host,
 * the sRGB table (main.c:85-88) and the filter weights (main.c:306-319).  Compiled without contraction. */
#include "vkr_internal.h"
#include "vkr_texture_conversion.h"
#include "../glibc_math.h"

VKR_API void evaluate_texture_conversion_powf(float* out, const float* x, float y, uint64_t count) {
	for (uint64_t i = 0; i != count; ++i) out[i] = gm_powf(x[i], y);
}

VKR_API void get_texture_conversion_tables(float tables[512]) {
	for (uint32_t b = 0; b != 256; ++b) {
		float s = b * (1.0f / 255.0f);
		tables[b] = (s <= 0.04045f) ? (s * (1.0f / 12.92f)) : gm_powf(s * (1.0f / 1.055f) + 0.055f / 1.055f, 2.4f);
		tables[256 + b] = s;
	}
}

/* The weights for which expf() of the reference's C library (glibc 2.35) and (float) exp() disagree, all levels up to
   VKR_TEXTURE_CONVERSION_MAX_LEVEL searched: {level, j, the bits expf() gave}.  The rule takes the reference's bits. */
static const uint32_t weight_exceptions[][3] = {
	{11, 708, 0x3DD162FBu}, {11, 1476, 0x3EF9C792u}, {11, 1626, 0x3F18F0D1u}, {11, 2150, 0x3F6E95E1u},
	{11, 2765, 0x3F6E95E1u}, {11, 3289, 0x3F18F0D1u}, {11, 3439, 0x3EF9C792u}, {11, 4207, 0x3DD162FBu},
	{12, 109, 0x3C5D9AD4u}, {12, 1833, 0x3E2E7282u}, {12, 3922, 0x3F5501DFu}, {12, 5909, 0x3F5501DFu},
	{12, 7998, 0x3E2E7282u}, {12, 9722, 0x3C5D9AD4u}};

/* w[j] of the header before normalisation */
static float unnormalised_weight(uint32_t level, int32_t j, float gaussian_factor, float filter_center) {
	for (uint32_t i = 0; i != VKR_COUNT_OF(weight_exceptions); ++i)
		if (weight_exceptions[i][0] == level && weight_exceptions[i][1] == (uint32_t) j) return gm_float(weight_exceptions[i][2]);
	float argument = gaussian_factor * (j - filter_center) * (j - filter_center);
	return (float) exp((double) argument);
}

VKR_API uint32_t get_texture_filter_weights(float* weights, uint32_t capacity, uint32_t level) {
	if (level < 1 || level > VKR_TEXTURE_CONVERSION_MAX_LEVEL) return 0;
	int32_t filter_scale = 1 << level;
	float standard_deviation = 0.4f * filter_scale;
	float gaussian_factor = -0.5f / (standard_deviation * standard_deviation);
	int32_t filter_extent = (int32_t) ceilf(3.0f * standard_deviation);
	float filter_center = filter_extent - 0.5f;
	if (!weights) return (uint32_t) filter_extent;
	/* (the sum runs over all weights, whatever part of them the caller has room for) */
	float total_weight = 0.0f;
	for (int32_t j = 0; j != 2 * filter_extent; ++j) total_weight += unnormalised_weight(level, j, gaussian_factor, filter_center);
	float normalization = 1.0f / total_weight;
	for (int32_t j = 0; j != 2 * filter_extent && (uint32_t) j < capacity; ++j)
		weights[j] = unnormalised_weight(level, j, gaussian_factor, filter_center) * normalization;
	return (uint32_t) filter_extent;
}

VKR_API int write_converted_texture(const converted_texture_t* texture, const char* file_path) {
	if (!texture || !texture->payload || texture->mipmap_count < 1 || texture->mipmap_count > 32) {
		printf("There is no converted texture to write to %s.\n", file_path ? file_path : "(null)");
		return 1;
	}
	FILE* file = file_path ? fopen(file_path, "wb") : NULL;
	if (!file) {
		printf("Failed to open the output file: %s\n", file_path ? file_path : "(null)");
		return 1;
	}
	int32_t header[6] = {0xbc1bc1, 1, texture->mipmap_count, texture->width, texture->height, texture->format};
	int failed = fwrite(header, sizeof(int32_t), 6, file) != 6 || fwrite(&texture->payload_size, sizeof(uint64_t), 1, file) != 1;
	for (int32_t i = 0; i != texture->mipmap_count && !failed; ++i) {
		int32_t extent[2] = {texture->width >> i, texture->height >> i};
		uint64_t size_offset[2] = {texture->mipmap_sizes[i], texture->mipmap_offsets[i]};
		failed = fwrite(extent, sizeof(int32_t), 2, file) != 2 || fwrite(size_offset, sizeof(uint64_t), 2, file) != 2;
	}
	uint32_t eof_marker = 0xE0FE0F;
	failed = failed || fwrite(texture->payload, 1, texture->payload_size, file) != texture->payload_size
		|| fwrite(&eof_marker, sizeof(eof_marker), 1, file) != 1;
	failed |= fclose(file) != 0;
	if (failed) printf("Failed to write the texture file at path %s.\n", file_path);
	return failed;
}

VKR_API void free_converted_texture(converted_texture_t* texture) {
	free(texture->payload);
	memset(texture, 0, sizeof(*texture));
}
