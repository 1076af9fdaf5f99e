/* The host part of the JPEG encoder (include/vkr_jpeg.h): quantisation tables and descaling factors for a quality,
   Huffman code words from the specifications of ITU-T T.81 Annex K, the 607-byte file header, the worst-case size and
   the file writer.  The kernels are csrc/jpeg_encoder.hip. */
#include "vkr_jpeg_tables.h"
#include "vkr_internal.h"
#include <stdio.h>
#include <string.h>

/* T.81 Table K.1 and K.2, row by row */
static const uint8_t k_base_tables[2][64] = {
	{16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
	 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
	{17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
	 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

/* T.81 Tables K.3 - K.6 in the order of the DHT segment (DC 0, AC 0, DC 1, AC 1): codes per length 1 ... 16, then the
   symbols in order of increasing code length */
static const uint8_t k_code_counts[4][16] = {
	{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
	{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D},
	{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
	{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
static const uint8_t k_dc_symbols[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t k_ac_luminance_symbols[162] = {
	0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
	0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72,
	0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37,
	0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
	0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83,
	0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3,
	0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3,
	0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
	0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA};
static const uint8_t k_ac_chrominance_symbols[162] = {
	0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
	0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1,
	0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36,
	0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
	0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A,
	0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A,
	0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA,
	0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
	0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA};
static const uint8_t* const k_symbols[4] = {k_dc_symbols, k_ac_luminance_symbols, k_dc_symbols, k_ac_chrominance_symbols};
static const uint8_t k_class_and_id[4] = {0x00, 0x10, 0x01, 0x11};

static uint32_t symbol_count(uint32_t table) {
	uint32_t count = 0;
	for (uint32_t i = 0; i != 16; ++i) count += k_code_counts[table][i];
	return count;
}

void vkr_jpeg_zigzag_positions(uint8_t position[64]) {
	/* T.81 figure A.6: diagonals r + c = 0 ... 14, odd ones walked downwards, even ones upwards */
	uint32_t next = 0;
	for (uint32_t diagonal = 0; diagonal != 15; ++diagonal)
		for (uint32_t step = 0; step != 8; ++step) {
			uint32_t row = (diagonal & 1) ? step : 7 - step;
			if (diagonal < row || diagonal - row > 7) continue;
			position[8 * row + (diagonal - row)] = (uint8_t) next++;
		}
}

int vkr_jpeg_effective_quality(int32_t quality, uint32_t* effective) {
	if (quality == 0) quality = 90;
	int subsampled = quality <= 90;
	*effective = (uint32_t) (quality < 1 ? 1 : quality > 100 ? 100 : quality);
	return subsampled;
}

uint32_t vkr_jpeg_data_unit_count(uint32_t width, uint32_t height, int subsampled) {
	uint32_t mcu = subsampled ? 16 : 8;
	return ((width + mcu - 1) / mcu) * ((height + mcu - 1) / mcu) * (subsampled ? 6 : 3);
}

static int extent_is_valid(uint32_t width, uint32_t height) { return width != 0 && height != 0 && width <= 65535 && height <= 65535; }

void vkr_jpeg_make_tables(vkr_jpeg_tables_t* tables, uint32_t width, uint32_t height, int32_t quality) {
	memset(tables, 0, sizeof(*tables));
	uint32_t q;
	tables->subsampled = (uint32_t) vkr_jpeg_effective_quality(quality, &q);
	tables->quality = q;
	vkr_jpeg_zigzag_positions(tables->zigzag);
	int32_t s = q < 50 ? 5000 / (int32_t) q : 200 - 2 * (int32_t) q;
	static const float aan[8] = {1.0f, 1.387039845f, 1.306562965f, 1.175875602f, 1.0f, 0.785694958f, 0.541196100f, 0.275899379f};
	float a[8];
	for (uint32_t k = 0; k != 8; ++k) a[k] = aan[k] * 2.828427125f;
	uint8_t entries[2][64];
	for (uint32_t t = 0; t != 2; ++t)
		for (uint32_t i = 0; i != 64; ++i) {
			int32_t entry = ((int32_t) k_base_tables[t][i] * s + 50) / 100;
			entries[t][i] = (uint8_t) (entry < 1 ? 1 : entry > 255 ? 255 : entry);
			tables->factors[t][i] = 1.0f / (((float) entries[t][i] * a[i / 8]) * a[i % 8]);
		}
	/* code words: T.81 Annex C */
	for (uint32_t t = 0; t != 4; ++t) {
		uint32_t code = 0, k = 0;
		for (uint32_t length = 1; length <= 16; ++length) {
			for (uint32_t i = 0; i != k_code_counts[t][length - 1]; ++i) tables->codes[t][k_symbols[t][k++]] = (length << 16) | code++;
			code <<= 1;
		}
	}
	/* the header */
	uint8_t* h = tables->header;
	static const uint8_t app0_and_dqt[] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0, 0xFF, 0xDB, 0, 0x84};
	memcpy(h, app0_and_dqt, sizeof(app0_and_dqt)); h += sizeof(app0_and_dqt);
	for (uint32_t t = 0; t != 2; ++t) {
		*h++ = (uint8_t) t;
		for (uint32_t i = 0; i != 64; ++i) h[tables->zigzag[i]] = entries[t][i];
		h += 64;
	}
	const uint8_t sof0_and_dht[] = {0xFF, 0xC0, 0, 17, 8, (uint8_t) (height >> 8), (uint8_t) height, (uint8_t) (width >> 8), (uint8_t) width, 3,
	                                1, (uint8_t) (tables->subsampled ? 0x22 : 0x11), 0, 2, 0x11, 1, 3, 0x11, 1, 0xFF, 0xC4, 0x01, 0xA2};
	memcpy(h, sof0_and_dht, sizeof(sof0_and_dht)); h += sizeof(sof0_and_dht);
	for (uint32_t t = 0; t != 4; ++t) {
		*h++ = k_class_and_id[t];
		memcpy(h, k_code_counts[t], 16); h += 16;
		uint32_t count = symbol_count(t);
		memcpy(h, k_symbols[t], count); h += count;
	}
	static const uint8_t sos[] = {0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
	memcpy(h, sos, sizeof(sos)); h += sizeof(sos);
	if (h - tables->header != VKR_JPEG_HEADER_SIZE) printf("The JPEG header has %d bytes instead of %d.\n", (int) (h - tables->header), VKR_JPEG_HEADER_SIZE);
}

uint64_t vkr_jpeg_worst_case_bits(uint32_t data_unit_count) {
	vkr_jpeg_tables_t tables;
	vkr_jpeg_make_tables(&tables, 8, 8, 100);
	/* the longest code with its extra bits: the category is the symbol of a DC table, the low nibble of one of an AC table */
	uint32_t longest[2] = {0, 0};
	for (uint32_t t = 0; t != 4; ++t)
		for (uint32_t symbol = 0; symbol != 256; ++symbol) {
			uint32_t length = tables.codes[t][symbol] >> 16, bits = length + ((t & 1) ? (symbol & 15) : symbol);
			if (length && bits > longest[t & 1]) longest[t & 1] = bits;
		}
	return (uint64_t) data_unit_count * (longest[0] + 63 * longest[1]);
}

uint64_t get_jpeg_capacity(uint32_t width, uint32_t height, int32_t quality) {
	if (!extent_is_valid(width, height)) return 0;
	uint32_t q;
	int subsampled = vkr_jpeg_effective_quality(quality, &q);
	uint64_t bits = vkr_jpeg_worst_case_bits(vkr_jpeg_data_unit_count(width, height, subsampled));
	return VKR_JPEG_HEADER_SIZE + 2 * ((bits + 7) / 8 + 1) + 2;
}

uint32_t get_jpeg_stuffing_chunk_size(void) { return VKR_JPEG_STUFFING_CHUNK; }

int get_jpeg_header(uint8_t header[VKR_JPEG_HEADER_SIZE], uint32_t width, uint32_t height, int32_t quality) {
	if (!extent_is_valid(width, height)) {
		printf("A JPEG is between 1 x 1 and 65535 x 65535 pixels, not %u x %u.\n", width, height);
		return 1;
	}
	vkr_jpeg_tables_t tables;
	vkr_jpeg_make_tables(&tables, width, height, quality);
	memcpy(header, tables.header, VKR_JPEG_HEADER_SIZE);
	return 0;
}

int write_jpeg(const char* path, const uint8_t* bytes, uint64_t size) { return vkr_write_file(path, bytes, size); }
