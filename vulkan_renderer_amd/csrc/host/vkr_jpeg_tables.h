/* What the host part (jpeg_tables.c) makes for the kernels of the JPEG encoder (../jpeg_encoder.hip). */
#ifndef VKR_JPEG_TABLES_H
#define VKR_JPEG_TABLES_H
#include "vkr_jpeg.h"

#ifdef __cplusplus
extern "C" {
#endif

/*! Everything that depends on extent and quality alone; uploaded as it is */
typedef struct vkr_jpeg_tables_s {
	/*! descaling factors in row-major order: luminance, chrominance */
	float factors[2][64];
	/*! length << 16 | code word per symbol, 0 for a symbol without code: DC 0, AC 0, DC 1, AC 1 */
	uint32_t codes[4][256];
	/*! the zig-zag position of the coefficient 8 row + column */
	uint8_t zigzag[64];
	uint8_t header[VKR_JPEG_HEADER_SIZE + 1];
	uint32_t quality, subsampled;
} vkr_jpeg_tables_t;

void vkr_jpeg_make_tables(vkr_jpeg_tables_t* tables, uint32_t width, uint32_t height, int32_t quality);
void vkr_jpeg_zigzag_positions(uint8_t position[64]);
/*! whether chroma is subsampled; *effective gets the quality in 1 ... 100 */
int vkr_jpeg_effective_quality(int32_t quality, uint32_t* effective);
uint32_t vkr_jpeg_data_unit_count(uint32_t width, uint32_t height, int subsampled);
/*! the bits of the longest entropy-coded segment of that many data units, before fill and stuffing */
uint64_t vkr_jpeg_worst_case_bits(uint32_t data_unit_count);

#ifdef __cplusplus
}
#endif

#endif
