// Frames as baseline JPEG files on the device (include/vkr_jpeg.h states the rule; csrc/host/jpeg_tables.c makes the
// tables and the header).  One encode is a chain of kernels on the caller's stream, without a host wait in between:
//   k_jpeg_coefficients     colour transform, chroma means, both DCT passes, quantisation: int16 [data unit][64], zig-zag
//   k_jpeg_lengths          the bits of every data unit (its DC needs its predecessor's); hipcub exclusive sum, 64 bit
//   k_jpeg_zero_words       zeroes the words the bits will land in
//   k_jpeg_pack             every data unit writes its bits at its offset
//   k_jpeg_count_stuffing   0xFF bytes per chunk of VKR_JPEG_STUFFING_CHUNK bytes; hipcub exclusive sum
//   k_jpeg_stuff            header, bytes with the inserted zeros, EOI, size word
//   k_copy_record_out       (output_slots.hip) the size record and that many bytes into the slot's pinned staging memory
// This unit is compiled without contraction whatever the arithmetic mode of the pass: the bytes are the interface.
#include "vkr_jpeg.h"
#include "host/vkr_jpeg_tables.h"
#include "output_slots.h"
#include <hipcub/hipcub.hpp>

namespace {

constexpr uint32_t kChunk = VKR_JPEG_STUFFING_CHUNK;

struct jpeg_geometry {
	uint32_t width, height, mcus_x, data_unit_count, subsampled;
};

// ---- coefficients ----------------------------------------------------------------------------------------------------

template <bool DWORD>
__device__ inline void load_rgb(const uint8_t* pixels, uint64_t stride, uint32_t channels, const jpeg_geometry& geo, uint32_t x, uint32_t y, float& r, float& g, float& b) {
	// beyond the image: the last column, the last row
	x = min(x, geo.width - 1);
	y = min(y, geo.height - 1);
	const uint8_t* p = pixels + (uint64_t) y * stride + (uint64_t) x * channels;
	if (DWORD) {
		uint32_t rgba = *(const uint32_t*) p;
		r = (float) (rgba & 255u); g = (float) ((rgba >> 8) & 255u); b = (float) ((rgba >> 16) & 255u);
	}
	else {
		r = (float) p[0]; g = (float) p[1]; b = (float) p[2];
	}
}

__device__ inline float colour_component(float r, float g, float b, uint32_t component) {
	if (component == 0) return ((0.299f * r + 0.587f * g) + 0.114f * b) - 128.0f;
	if (component == 1) return (-0.16874f * r - 0.33126f * g) + 0.5f * b;
	return (0.5f * r - 0.41869f * g) - 0.08131f * b;
}

// one pass of the forward transform over eight values, in the association of sums that include/vkr_jpeg.h gives
__device__ inline void dct_pass(float& d0, float& d1, float& d2, float& d3, float& d4, float& d5, float& d6, float& d7) {
	float t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
	float e0 = t0 + t3, e3 = t0 - t3, e1 = t1 + t2, e2 = t1 - t2;
	d0 = e0 + e1;
	d4 = e0 - e1;
	float z1 = (e2 + e3) * 0.707106781f;
	d2 = e3 + z1;
	d6 = e3 - z1;
	float o0 = t4 + t5, o1 = t5 + t6, o2 = t6 + t7;
	float z5 = (o0 - o2) * 0.382683433f;
	float z2 = o0 * 0.541196100f + z5;
	float z4 = o2 * 1.306562965f + z5;
	float z3 = o1 * 0.707106781f;
	float z11 = t7 + z3, z13 = t7 - z3;
	d5 = z13 + z2;
	d3 = z13 - z2;
	d1 = z11 + z4;
	d7 = z11 - z4;
}

// the component of a data unit in scan order and where in the frame its 8 x 8 (Y) or 16 x 16 (subsampled chroma) pixels begin
__device__ inline uint32_t locate_data_unit(const jpeg_geometry& geo, uint32_t unit, uint32_t& x0, uint32_t& y0) {
	uint32_t per_mcu = geo.subsampled ? 6 : 3, mcu = unit / per_mcu, k = unit - mcu * per_mcu;
	uint32_t mcu_x = mcu % geo.mcus_x, mcu_y = mcu / geo.mcus_x;
	if (!geo.subsampled) {
		x0 = mcu_x * 8; y0 = mcu_y * 8;
		return k;
	}
	x0 = mcu_x * 16 + (k < 4 ? (k & 1) * 8 : 0);
	y0 = mcu_y * 16 + (k < 4 ? (k >> 1) * 8 : 0);
	return k < 4 ? 0 : k - 3;
}

// Eight lanes per data unit: a lane loads and transforms one row, the rows change into columns through LDS, the lane
// transforms one column and stores its eight coefficients.  (One lane per data unit with all 64 samples in registers was
// 2.7 times slower at 1920 x 1080 and 3.3 times at 3840 x 2160: 765 waves of 95 VGPRs for 1024 SIMDs)
template <bool DWORD>
__global__ void __launch_bounds__(256) k_jpeg_coefficients(const uint8_t* pixels, uint64_t stride, uint32_t channels, jpeg_geometry geo, const vkr_jpeg_tables_t* tables, int16_t* coefficients) {
	// (rows of nine floats: the column reads of eight lanes fall into eight banks)
	__shared__ float tile[32][8][9];
	uint32_t row = threadIdx.x & 7, local = threadIdx.x >> 3, unit = blockIdx.x * 32 + local;
	bool active = unit < geo.data_unit_count;
	uint32_t x0 = 0, y0 = 0, component = active ? locate_data_unit(geo, unit, x0, y0) : 0;
	float d[8];
	if (active) {
		if (geo.subsampled && component != 0) {
#pragma unroll
			for (uint32_t x = 0; x != 8; ++x) {
				float a[4];
#pragma unroll
				for (uint32_t i = 0; i != 4; ++i) {
					float r, g, b;
					load_rgb<DWORD>(pixels, stride, channels, geo, x0 + 2 * x + (i & 1), y0 + 2 * row + (i >> 1), r, g, b);
					a[i] = colour_component(r, g, b, component);
				}
				d[x] = (((a[0] + a[1]) + a[2]) + a[3]) * 0.25f;
			}
		}
		else {
#pragma unroll
			for (uint32_t x = 0; x != 8; ++x) {
				float r, g, b;
				load_rgb<DWORD>(pixels, stride, channels, geo, x0 + x, y0 + row, r, g, b);
				d[x] = colour_component(r, g, b, component);
			}
		}
		dct_pass(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7]);
#pragma unroll
		for (uint32_t x = 0; x != 8; ++x) tile[local][row][x] = d[x];
	}
	__syncthreads();
	if (!active) return;
	// the lane's column is the one with its row's number
#pragma unroll
	for (uint32_t y = 0; y != 8; ++y) d[y] = tile[local][y][row];
	dct_pass(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7]);
	const float* factors = tables->factors[component ? 1 : 0];
	int16_t* out = coefficients + (uint64_t) unit * 64;
#pragma unroll
	for (uint32_t y = 0; y != 8; ++y) {
		float v = d[y] * factors[8 * y + row];
		out[tables->zigzag[8 * y + row]] = (int16_t) (int32_t) (v < 0.0f ? v - 0.5f : v + 0.5f);
	}
}

// ---- entropy coding ---------------------------------------------------------------------------------------------------

// the data unit whose DC value a data unit is coded against, -1 for the first of a component
__device__ inline int64_t dc_predecessor(const jpeg_geometry& geo, uint32_t unit, uint32_t& component) {
	if (!geo.subsampled) {
		component = unit % 3;
		return (int64_t) unit - 3;
	}
	uint32_t k = unit % 6;
	component = k < 4 ? 0 : k - 3;
	if (k >= 4) return (int64_t) unit - 6;
	// the Y units of an MCU follow each other; the first follows the fourth of the MCU before
	return (int64_t) unit - (k ? 1 : 3);
}

__device__ inline uint32_t category_of(int32_t value) {
	uint32_t magnitude = (uint32_t) (value < 0 ? -value : value);
	return magnitude ? 32u - (uint32_t) __clz(magnitude) : 0u;
}

// a value with its Huffman code in front: (code << category | low bits of value or value - 1, bit count)
template <typename Sink>
__device__ inline void put_coded(Sink& sink, uint32_t table_entry, int32_t value, uint32_t category) {
	uint32_t extra = (uint32_t) (value < 0 ? value - 1 : value) & ((1u << category) - 1u);
	sink.put(((table_entry & 0xFFFFu) << category) | extra, (table_entry >> 16) + category);
}

// Walks one data unit as T.81 F.1.2 says and hands every code to sink.put(bits, count), count <= 27.  codes: the four
// tables of vkr_jpeg_tables_t in LDS.
template <typename Sink>
__device__ inline void code_data_unit(const jpeg_geometry& geo, const int16_t* coefficients, uint32_t unit, const uint32_t* codes, Sink& sink) {
	uint32_t component;
	int64_t predecessor = dc_predecessor(geo, unit, component);
	const uint32_t* dc_codes = codes + (component ? 512 : 0);
	const uint32_t* ac_codes = dc_codes + 256;
	const uint4* source = (const uint4*) (coefficients + (uint64_t) unit * 64);
	int32_t previous_dc = predecessor >= 0 ? (int32_t) coefficients[(uint64_t) predecessor * 64] : 0;
	uint32_t run = 0;
	for (uint32_t q = 0; q != 8; ++q) {
		uint4 packed = source[q];
		uint32_t words[4] = {packed.x, packed.y, packed.z, packed.w};
#pragma unroll
		for (uint32_t j = 0; j != 8; ++j) {
			int32_t value = (int32_t) (int16_t) (words[j >> 1] >> ((j & 1) * 16));
			if (q == 0 && j == 0) {
				int32_t difference = value - previous_dc;
				uint32_t category = category_of(difference);
				put_coded(sink, dc_codes[category & 255u], difference, category);
			}
			else if (value == 0) ++run;
			else {
				for (; run >= 16; run -= 16) sink.put(ac_codes[0xF0] & 0xFFFFu, ac_codes[0xF0] >> 16);
				uint32_t category = category_of(value);
				put_coded(sink, ac_codes[((run << 4) + category) & 255u], value, category);
				run = 0;
			}
		}
	}
	// EOB unless coefficient 63 is nonzero
	if (run) sink.put(ac_codes[0] & 0xFFFFu, ac_codes[0] >> 16);
}

__device__ inline void load_codes(uint32_t* shared_codes, const vkr_jpeg_tables_t* tables) {
	for (uint32_t i = threadIdx.x; i < 1024; i += blockDim.x) shared_codes[i] = (&tables->codes[0][0])[i];
	__syncthreads();
}

struct bit_counter {
	uint32_t bits;
	__device__ void put(uint32_t, uint32_t count) { bits += count; }
};

// lengths[unit] = the bits of the data unit, lengths[data_unit_count] = 0: the exclusive sum over all of them ends with the total
__global__ void __launch_bounds__(256) k_jpeg_lengths(const int16_t* coefficients, jpeg_geometry geo, const vkr_jpeg_tables_t* tables, uint64_t* lengths) {
	__shared__ uint32_t codes[1024];
	load_codes(codes, tables);
	uint32_t unit = blockIdx.x * 256 + threadIdx.x;
	if (unit > geo.data_unit_count) return;
	bit_counter counter = {0};
	if (unit < geo.data_unit_count) code_data_unit(geo, coefficients, unit, codes, counter);
	lengths[unit] = counter.bits;
}

__global__ void __launch_bounds__(256) k_jpeg_zero_words(uint32_t* words, const uint64_t* total_bits, uint64_t word_capacity) {
	uint64_t count = min(*total_bits / 32 + 1, word_capacity);
	for (uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x; i < count; i += (uint64_t) gridDim.x * 256) words[i] = 0;
}

// Bits most significant first into 32-bit words.  A word that a data unit covers completely is stored; the word it
// begins in the middle of and the word it ends in the middle of are shared with its neighbours and get atomicOr.
struct bit_writer {
	uint32_t* words;
	uint64_t index;
	uint32_t filled, current;
	bool shared_word;
	__device__ void put(uint32_t bits, uint32_t count) {
		while (count) {
			uint32_t room = 32 - filled, take = count < room ? count : room;
			current |= ((bits >> (count - take)) & ((1u << take) - 1u)) << (room - take);
			filled += take;
			count -= take;
			if (filled == 32) {
				if (shared_word) atomicOr(words + index, current);
				else words[index] = current;
				++index; current = 0; filled = 0; shared_word = false;
			}
		}
	}
	__device__ void finish() {
		if (filled) atomicOr(words + index, current);
	}
};

__global__ void __launch_bounds__(256) k_jpeg_pack(const int16_t* coefficients, jpeg_geometry geo, const vkr_jpeg_tables_t* tables, const uint64_t* offsets, uint32_t* words) {
	__shared__ uint32_t codes[1024];
	load_codes(codes, tables);
	uint32_t unit = blockIdx.x * 256 + threadIdx.x;
	if (unit >= geo.data_unit_count) return;
	uint64_t offset = offsets[unit];
	bit_writer writer = {words, offset >> 5, (uint32_t) (offset & 31), 0u, (offset & 31) != 0};
	code_data_unit(geo, coefficients, unit, codes, writer);
	writer.finish();
}

// ---- stuffing ---------------------------------------------------------------------------------------------------------

// the bytes of chunk `chunk` of the packed stream that exist, the last one of the stream filled with ones
template <typename Visit>
__device__ inline void visit_chunk(const uint32_t* words, uint64_t chunk, uint64_t total_bits, Visit& visit) {
	uint64_t packed_bytes = (total_bits + 7) / 8;
	uint32_t fill = (total_bits & 7) ? (0xFFu >> (total_bits & 7)) : 0u;
	const uint4* source = (const uint4*) (words + chunk * (kChunk / 4));
	for (uint32_t q = 0; q != kChunk / 16; ++q) {
		uint64_t first = chunk * kChunk + q * 16;
		if (first >= packed_bytes) break;
		uint4 packed = source[q];
		uint32_t four[4] = {packed.x, packed.y, packed.z, packed.w};
#pragma unroll
		for (uint32_t j = 0; j != 16; ++j) {
			uint64_t at = first + j;
			if (at < packed_bytes) {
				uint32_t byte = (four[j >> 2] >> (24 - 8 * (j & 3))) & 255u;
				if (at == packed_bytes - 1) byte |= fill;
				visit.byte(byte);
			}
		}
	}
}

struct stuffing_counter {
	uint32_t count;
	__device__ void byte(uint32_t value) { count += value == 255u; }
};

// counts[chunk] for chunk <= chunk_capacity (0 behind the end of the stream): the exclusive sum gives every chunk the
// zeros inserted in front of it
__global__ void __launch_bounds__(256) k_jpeg_count_stuffing(const uint32_t* words, const uint64_t* total_bits, uint32_t* counts, uint64_t chunk_capacity) {
	uint64_t chunk = (uint64_t) blockIdx.x * 256 + threadIdx.x;
	if (chunk > chunk_capacity) return;
	stuffing_counter counter = {0};
	if (chunk < chunk_capacity) visit_chunk(words, chunk, *total_bits, counter);
	counts[chunk] = counter.count;
}

struct stuffing_writer {
	uint8_t* out;
	uint64_t at, capacity;
	__device__ void put(uint32_t value) {
		if (at < capacity) out[at] = (uint8_t) value;
		++at;
	}
	__device__ void byte(uint32_t value) {
		put(value);
		if (value == 255u) put(0);
	}
};

// Lane t writes byte t of the header and chunk t of the stream; the lane of the last chunk adds EOI and the size word.
// Nothing at or beyond out + capacity is written.
__global__ void __launch_bounds__(256) k_jpeg_stuff(const uint32_t* words, const uint64_t* total_bits_pointer, const uint32_t* chunk_offsets, const vkr_jpeg_tables_t* tables,
                                                   uint8_t* out, uint64_t capacity, uint64_t* size_word, uint64_t chunk_capacity) {
	uint64_t chunk = (uint64_t) blockIdx.x * 256 + threadIdx.x;
	if (chunk < VKR_JPEG_HEADER_SIZE && chunk < capacity) out[chunk] = tables->header[chunk];
	uint64_t total_bits = *total_bits_pointer, packed_bytes = (total_bits + 7) / 8;
	if (chunk >= chunk_capacity || chunk * kChunk >= packed_bytes) return;
	stuffing_writer writer = {out, VKR_JPEG_HEADER_SIZE + chunk * kChunk + chunk_offsets[chunk], capacity};
	visit_chunk(words, chunk, total_bits, writer);
	if ((chunk + 1) * kChunk >= packed_bytes) {
		writer.put(0xFF);
		writer.put(0xD9);
		*size_word = writer.at;
	}
}

// ---- the encoder ------------------------------------------------------------------------------------------------------

// the scratch memory of a slot besides what output_slots.h keeps
struct jpeg_slot {
	int16_t* coefficients;
	uint64_t *lengths, *offsets;
	uint32_t *words, *chunk_counts, *chunk_offsets;
};

struct jpeg_state {
	// (what its slots share: the vkr_jpeg_tables_t)
	output_slots out;
	jpeg_geometry geo;
	uint64_t word_capacity, chunk_capacity;
	jpeg_slot slots[kMaxOutputSlots];
};

output_slots* slots_of(const jpeg_encoder_t* encoder) { return encoder && encoder->state ? &((jpeg_state*) encoder->state)->out : NULL; }

void lay_out_slot(output_carver& carve, void* jpeg_state_pointer, uint32_t slot_index) {
	jpeg_state* state = (jpeg_state*) jpeg_state_pointer;
	jpeg_slot& slot = state->slots[slot_index];
	size_t units = state->geo.data_unit_count;
	carve.take(slot.coefficients, units * 64);
	carve.take(slot.lengths, units + 1);
	carve.take(slot.offsets, units + 1);
	carve.take(slot.words, state->word_capacity);
	carve.take(slot.chunk_counts, state->chunk_capacity + 1);
	carve.take(slot.chunk_offsets, state->chunk_capacity + 1);
}

int enqueue_encode(jpeg_encoder_t* encoder, uint32_t slot_index, const void* device_pixels, uint32_t channel_count, uint64_t row_stride_bytes,
                   uint8_t* out, uint64_t capacity, uint64_t* size_word, bool copy_out, void* stream_or_null) {
	jpeg_state* state = (jpeg_state*) encoder->state;
	if (!state || !device_pixels || (channel_count != 3 && channel_count != 4)) {
		printf("A JPEG encode needs an encoder and device pixels of 3 or 4 channels.\n");
		return 1;
	}
	if (row_stride_bytes == 0) row_stride_bytes = (uint64_t) encoder->width * channel_count;
	if (row_stride_bytes < (uint64_t) encoder->width * channel_count) {
		printf("A row stride of %llu bytes is less than a row of %u pixels of %u channels.\n", (unsigned long long) row_stride_bytes, encoder->width, channel_count);
		return 1;
	}
	hipStream_t stream;
	if (begin_output_enqueue(&state->out, slot_index, stream_or_null, &stream)) return 1;
	const jpeg_slot& slot = state->slots[slot_index];
	uint8_t* scan_storage = state->out.slots[slot_index].scan_storage;
	const vkr_jpeg_tables_t* tables = (const vkr_jpeg_tables_t*) state->out.shared;
	const jpeg_geometry& geo = state->geo;
	uint32_t units = geo.data_unit_count;
	bool dwords = channel_count == 4 && ((uintptr_t) device_pixels % 4 == 0) && row_stride_bytes % 4 == 0;
	if (dwords) k_jpeg_coefficients<true><<<block_count(units, 32), 256, 0, stream>>>((const uint8_t*) device_pixels, row_stride_bytes, channel_count, geo, tables, slot.coefficients);
	else k_jpeg_coefficients<false><<<block_count(units, 32), 256, 0, stream>>>((const uint8_t*) device_pixels, row_stride_bytes, channel_count, geo, tables, slot.coefficients);
	k_jpeg_lengths<<<block_count((uint64_t) units + 1, 256), 256, 0, stream>>>(slot.coefficients, geo, tables, slot.lengths);
	size_t scan_bytes = state->out.scan_bytes;
	if (hip_failed(hipcub::DeviceScan::ExclusiveSum(scan_storage, scan_bytes, slot.lengths, slot.offsets, (int) (units + 1), stream), "summing the lengths of the data units")) return 1;
	const uint64_t* total_bits = slot.offsets + units;
	k_jpeg_zero_words<<<256, 256, 0, stream>>>(slot.words, total_bits, state->word_capacity);
	k_jpeg_pack<<<block_count(units, 256), 256, 0, stream>>>(slot.coefficients, geo, tables, slot.offsets, slot.words);
	k_jpeg_count_stuffing<<<block_count(state->chunk_capacity + 1, 256), 256, 0, stream>>>(slot.words, total_bits, slot.chunk_counts, state->chunk_capacity);
	scan_bytes = state->out.scan_bytes;
	if (hip_failed(hipcub::DeviceScan::ExclusiveSum(scan_storage, scan_bytes, slot.chunk_counts, slot.chunk_offsets, (int) (state->chunk_capacity + 1), stream), "summing the stuffed bytes")) return 1;
	uint64_t lanes = state->chunk_capacity > VKR_JPEG_HEADER_SIZE ? state->chunk_capacity : VKR_JPEG_HEADER_SIZE;
	k_jpeg_stuff<<<block_count(lanes, 256), 256, 0, stream>>>(slot.words, total_bits, slot.chunk_offsets, tables, out, capacity, size_word, state->chunk_capacity);
	return finish_output_enqueue(&state->out, slot_index, stream, copy_out ? 128 : 0);
}

}  // namespace

extern "C" void destroy_jpeg_encoder(jpeg_encoder_t* encoder) {
	jpeg_state* state = encoder ? (jpeg_state*) encoder->state : NULL;
	if (state) {
		destroy_output_slots(&state->out);
		free(state);
	}
	if (encoder) memset(encoder, 0, sizeof(*encoder));
}

extern "C" int create_jpeg_encoder(jpeg_encoder_t* encoder, const device_t* device, uint32_t width, uint32_t height, int32_t quality, uint32_t slot_count) {
	memset(encoder, 0, sizeof(*encoder));
	if (check_output_arguments("JPEG", device, width, height, slot_count)) return 1;
	jpeg_state* state = (jpeg_state*) calloc(1, sizeof(jpeg_state));
	vkr_jpeg_tables_t* tables = (vkr_jpeg_tables_t*) malloc(sizeof(vkr_jpeg_tables_t));
	if (!state || !tables) {
		printf("Out of memory creating a JPEG encoder.\n");
		free(state); free(tables);
		return 1;
	}
	vkr_jpeg_make_tables(tables, width, height, quality);
	encoder->width = width; encoder->height = height;
	encoder->quality = tables->quality; encoder->subsampled = tables->subsampled;
	encoder->slot_count = slot_count;
	encoder->data_unit_count = vkr_jpeg_data_unit_count(width, height, (int) tables->subsampled);
	encoder->capacity = get_jpeg_capacity(width, height, quality);
	encoder->state = state;
	uint32_t mcu = tables->subsampled ? 16 : 8, units = encoder->data_unit_count;
	state->geo = {width, height, (width + mcu - 1) / mcu, units, tables->subsampled};
	// the packed stream: whole chunks, so that the stuffing kernels load sixteen bytes at a time without a guard
	uint64_t packed_bytes = (vkr_jpeg_worst_case_bits(units) + 7) / 8 + 1;
	state->chunk_capacity = (packed_bytes + kChunk - 1) / kChunk;
	state->word_capacity = state->chunk_capacity * (kChunk / 4);
	size_t lengths_bytes = 0, counts_bytes = 0;
	int failed = hip_failed(hipcub::DeviceScan::ExclusiveSum(NULL, lengths_bytes, (uint64_t*) NULL, (uint64_t*) NULL, (int) (units + 1), (hipStream_t) device->stream), "sizing the sum of the lengths")
		|| hip_failed(hipcub::DeviceScan::ExclusiveSum(NULL, counts_bytes, (uint32_t*) NULL, (uint32_t*) NULL, (int) (state->chunk_capacity + 1), (hipStream_t) device->stream), "sizing the sum of the stuffed bytes")
		|| create_output_slots(&state->out, "JPEG", device, slot_count, encoder->capacity, 0, lengths_bytes > counts_bytes ? lengths_bytes : counts_bytes, tables, sizeof(vkr_jpeg_tables_t), lay_out_slot, state);
	free(tables);
	if (failed) destroy_jpeg_encoder(encoder);
	return failed;
}

extern "C" int begin_jpeg_encode(jpeg_encoder_t* encoder, uint32_t slot, const void* device_pixels, uint32_t channel_count, uint64_t row_stride_bytes, void* stream) {
	if (check_output_slot(slots_of(encoder), slot)) return 1;
	uint8_t* record = slots_of(encoder)->slots[slot].record;
	return enqueue_encode(encoder, slot, device_pixels, channel_count, row_stride_bytes, record + 16, encoder->capacity, (uint64_t*) record, true, stream);
}

extern "C" int end_jpeg_encode(jpeg_encoder_t* encoder, uint32_t slot, const uint8_t** bytes, uint64_t* size) { return end_output_encode(slots_of(encoder), slot, bytes, size); }

extern "C" int encode_jpeg(jpeg_encoder_t* encoder, const void* device_pixels, uint32_t channel_count, uint64_t row_stride_bytes, const uint8_t** bytes, uint64_t* size) {
	return begin_jpeg_encode(encoder, 0, device_pixels, channel_count, row_stride_bytes, NULL) || end_jpeg_encode(encoder, 0, bytes, size);
}

extern "C" int encode_jpeg_on_device(jpeg_encoder_t* encoder, const void* device_pixels, uint32_t channel_count, uint64_t row_stride_bytes,
                                     void* device_out, uint64_t capacity, uint64_t* device_size_word, void* stream) {
	if (check_output_slot(slots_of(encoder), 0)) return 1;
	if (!device_out || !device_size_word) {
		printf("encode_jpeg_on_device() needs device memory for the file and for its size.\n");
		return 1;
	}
	return enqueue_encode(encoder, 0, device_pixels, channel_count, row_stride_bytes, (uint8_t*) device_out, capacity, device_size_word, false, stream);
}
