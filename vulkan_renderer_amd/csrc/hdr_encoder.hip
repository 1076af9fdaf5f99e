// Frames as Radiance RGBE files on the device (include/vkr_hdr.h states the rule).  One encode is a chain of kernels on
// the caller's stream, without a host wait in between.  For run-length coded widths, one workgroup per row:
//   k_hdr_row_sizes      floats -> RGBE dwords (kept for the second pass), the coded size of the row's four planes
//   hipcub exclusive sum, 64 bit, over the rows
//   k_hdr_write_rows     header, scanline headers, the coded planes at their offsets, size word
// for the other widths k_hdr_raw alone: header, RGBE quadruples, size word.  Then
//   k_copy_record_out    (output_slots.hip) the size record and that many bytes into the slot's pinned staging memory
// The coding exists once, code_row<Load, Sink>: the first pass runs it with a sink that drops the bytes and keeps the
// positions, the second with one that stores them, so that sizes and bytes cannot disagree.
// This unit is compiled without contraction whatever the arithmetic mode of the pass: the bytes are the interface.
#include "vkr_hdr.h"
#include "output_slots.h"
#include <hip/hip_fp16.h>
#include <hipcub/hipcub.hpp>
#include <float.h>

namespace {

constexpr uint32_t kChunk = VKR_HDR_CHUNK;
constexpr uint32_t kSegment = VKR_HDR_SEGMENT;
// pixels staged besides a segment: the left neighbour of its first one, and three behind it (whether the element
// behind a chunk is part of a run depends on the three elements that follow the chunk)
constexpr uint32_t kBefore = 1, kBehind = 3;
constexpr uint32_t kStaged = kBefore + kSegment + kBehind;
static_assert(kChunk == 64 && kSegment % kChunk == 0, "a chunk is what one wave ballots over");

// ---- pixels -----------------------------------------------------------------------------------------------------------

struct hdr_source {
	const uint8_t* pixels;
	uint64_t stride;
	uint32_t channels, through_half;
	// rows of float4 that may be loaded as such
	uint32_t vectors;
};

__device__ inline float sanitise(float c, uint32_t through_half) {
	// (a NaN stays a NaN through the half and fails the comparison)
	if (through_half) c = __half2float(__float2half_rn(c));
	return c >= 0.0f ? (c > FLT_MAX ? FLT_MAX : c) : 0.0f;
}

// R | G << 8 | B << 16 | E << 24 of sanitised values
__device__ inline uint32_t rgbe_of(float r, float g, float b) {
	float inner = g > b ? g : b, m = r > inner ? r : inner;
	if (m < 1e-32f) return 0u;
	// m is positive and normal: m = f * 2^e, f in [0.5, 1), e = biased - 126; normalize = f * 256 / m = 2^(8 - e)
	uint32_t biased = __float_as_uint(m) >> 23;
	float normalize = __uint_as_float((261u - biased) << 23);
	return (uint32_t) (r * normalize) | ((uint32_t) (g * normalize) << 8) | ((uint32_t) (b * normalize) << 16) | (((biased + 2u) & 255u) << 24);
}

__device__ inline uint32_t load_rgbe(const hdr_source& source, uint32_t x, uint32_t y) {
	const float* p = (const float*) (source.pixels + (uint64_t) y * source.stride) + (uint64_t) x * source.channels;
	float r, g, b;
	if (source.vectors) {
		float4 v = *(const float4*) p;
		r = v.x; g = v.y; b = v.z;
	}
	else {
		r = p[0]; g = p[1]; b = p[2];
	}
	return rgbe_of(sanitise(r, source.through_half), sanitise(g, source.through_half), sanitise(b, source.through_half));
}

// ---- run-length coding ------------------------------------------------------------------------------------------------

// Codes the four component planes of one row, wave w of the workgroup of 256 plane w, and returns the coded size of the
// wave's plane.  load(x, own) gives the RGBE dword of pixel x of the row (own: x belongs to the segment being staged, not
// to its fringe); sink.put(at, byte) gets every byte of the coded plane with its position in it, each exactly once.
// staged: kStaged dwords of LDS.
// A wave walks its plane in chunks of 64 elements.  All that depends on other elements is a handful of 64-bit masks, the
// same in every lane: whether an element equals its left neighbour (one ballot, and one for the three elements behind
// the chunk), from that which elements are part of a run, where stretches and dumps start.  A lane finds the start of
// its stretch or dump as the highest set bit at or below it, or in what the wave carries from the chunks before.
template <typename Load, typename Sink>
__device__ inline uint32_t code_row(uint32_t width, Load& load, Sink& sink, uint32_t* staged) {
	const uint32_t lane = threadIdx.x & 63u, shift = 8u * (threadIdx.x >> 6);
	const uint64_t at_or_below = ~0ull >> (63u - lane), below = at_or_below >> 1;
	// carried from chunk to chunk: whether the element before the chunk equals its left neighbour; whether it is part of
	// a run (the row's border counts as one: a dump may start at element 0); where the last stretch and the last dump
	// started; the bytes coded so far
	uint64_t equal_before = 0, run_before = 1;
	uint32_t stretch_start = 0, dump_start = 0, position = 0;
	for (uint32_t first = 0; first < width; first += kSegment) {
		__syncthreads();
		for (uint32_t j = threadIdx.x; j < kStaged; j += 256u) {
			// (j == 0 of the first segment wraps around and is left out with the pixels behind the row)
			uint32_t x = first + j - kBefore;
			if (x < width) staged[j] = load(x, j >= kBefore && j < kBefore + kSegment);
		}
		__syncthreads();
		uint32_t count = min(kSegment, width - first);
		for (uint32_t base = 0; base < count; base += kChunk) {
			const uint32_t chunk_first = first + base, i = chunk_first + lane;
			// own[0] is element i and lies in `staged` for every lane, as own[-1] does; own[64] only for lanes 0 ... 2
			const uint32_t* own = staged + kBefore + base + lane;
			bool valid = i < width;
			uint32_t value = (own[0] >> shift) & 255u;
			bool equal = valid && i >= 1u && value == ((own[-1] >> shift) & 255u);
			bool equal_behind = lane < kBehind && i + kChunk < width && ((own[kChunk] >> shift) & 255u) == ((own[kChunk - 1u] >> shift) & 255u);
			uint64_t e0 = __ballot(equal), behind = __ballot(equal_behind);
			// e(i - 1), e(i + 1), e(i + 2), e(i + 3) at bit i
			uint64_t em1 = (e0 << 1) | equal_before, e1 = (e0 >> 1) | (behind << 63), e2 = (e0 >> 2) | (behind << 62), e3 = (e0 >> 3) | (behind << 61);
			// part of three equal bytes: as the last, the middle or the first of them; the same for element i + 1
			uint64_t run = (em1 & e0) | (e0 & e1) | (e1 & e2), run_next = (e0 & e1) | (e1 & e2) | (e2 & e3);
			uint64_t stretch_starts = ~e0, dump_starts = ~run & ((run << 1) | run_before);
			bool in_run = (run >> lane) & 1u;
			uint64_t starts = (in_run ? stretch_starts : dump_starts) & at_or_below;
			uint32_t start = starts ? chunk_first + 63u - (uint32_t) __clzll((long long) starts) : (in_run ? stretch_start : dump_start);
			// the offset in the run or dump, and what the element costs
			uint32_t k = i - start;
			uint32_t cost = !valid ? 0u : in_run ? (k % 127u == 0u ? 2u : 0u) : 1u + (k % 128u == 0u ? 1u : 0u);
			uint64_t ones = __ballot((cost & 1u) != 0u), twos = __ballot((cost & 2u) != 0u);
			uint32_t at = position + (uint32_t) __popcll(ones & below) + 2u * (uint32_t) __popcll(twos & below);
			if (valid) {
				if (in_run) {
					// the packet {128 + n, value} is written by its last element, which knows n
					uint32_t j = k % 127u;
					if (j == 126u || !((e1 >> lane) & 1u)) {
						uint32_t packet = j ? at - 2u : at;
						sink.put(packet, 129u + j);
						sink.put(packet + 1u, value);
					}
				}
				else {
					// every element of a dump writes its byte, the last one of a packet the count in front of it
					uint32_t j = k % 128u, data = at + (j == 0u ? 1u : 0u);
					sink.put(data, value);
					if (j == 127u || ((run_next >> lane) & 1u) || i == width - 1u) sink.put(data - j - 1u, j + 1u);
				}
			}
			position += (uint32_t) __popcll(ones) + 2u * (uint32_t) __popcll(twos);
			// (bits of lanes behind the row are set in both masks: only in the last chunk, after which nothing is carried)
			if (stretch_starts) stretch_start = chunk_first + 63u - (uint32_t) __clzll((long long) stretch_starts);
			if (dump_starts) dump_start = chunk_first + 63u - (uint32_t) __clzll((long long) dump_starts);
			equal_before = e0 >> 63;
			run_before = run >> 63;
		}
	}
	return position;
}

// the first pass: converts, keeps the RGBE dwords of the row for the second pass, and only wants the positions
struct float_loader {
	hdr_source source;
	uint32_t y;
	uint32_t* rgbe_row;
	__device__ uint32_t operator()(uint32_t x, bool own) {
		uint32_t rgbe = load_rgbe(source, x, y);
		if (own) rgbe_row[x] = rgbe;
		return rgbe;
	}
};

struct byte_counter {
	__device__ void put(uint32_t, uint32_t) {}
};

// plane_sizes[4 y + plane]; row_sizes[y] = 4 + the four of them, row_sizes[height] = 0: the exclusive sum ends with the total
__global__ void __launch_bounds__(256) k_hdr_row_sizes(hdr_source source, uint32_t width, uint32_t height, uint32_t* rgbe, uint32_t* plane_sizes, uint64_t* row_sizes) {
	__shared__ uint32_t staged[kStaged];
	__shared__ uint32_t sizes[4];
	uint32_t y = blockIdx.x, plane = threadIdx.x >> 6;
	float_loader load = {source, y, rgbe + (uint64_t) y * width};
	byte_counter counter;
	uint32_t size = code_row(width, load, counter, staged);
	if ((threadIdx.x & 63u) == 0u) {
		sizes[plane] = size;
		plane_sizes[4u * y + plane] = size;
	}
	__syncthreads();
	if (threadIdx.x == 0u) {
		row_sizes[y] = 4ull + sizes[0] + sizes[1] + sizes[2] + sizes[3];
		if (y == 0u) row_sizes[height] = 0ull;
	}
}

struct rgbe_loader {
	const uint32_t* rgbe_row;
	__device__ uint32_t operator()(uint32_t x, bool) { return rgbe_row[x]; }
};

// Nothing at or beyond out + capacity is written.
struct byte_writer {
	uint8_t* out;
	uint64_t base, capacity;
	__device__ void put(uint32_t at, uint32_t value) {
		uint64_t where = base + at;
		if (where < capacity) out[where] = (uint8_t) value;
	}
};

// The workgroup of row 0 also writes the header and the size word, wave 0 of every row the scanline header.
__global__ void __launch_bounds__(256) k_hdr_write_rows(const uint32_t* rgbe, uint32_t width, uint32_t height, const uint32_t* plane_sizes, const uint64_t* row_offsets,
                                                       const uint8_t* header, uint32_t header_size, uint8_t* out, uint64_t capacity, uint64_t* size_word) {
	__shared__ uint32_t staged[kStaged];
	uint32_t y = blockIdx.x, plane = threadIdx.x >> 6;
	uint64_t row_at = header_size + row_offsets[y];
	if (y == 0u) {
		if (threadIdx.x < header_size && threadIdx.x < capacity) out[threadIdx.x] = header[threadIdx.x];
		if (threadIdx.x == 0u) *size_word = header_size + row_offsets[height];
	}
	if (threadIdx.x < 4u && row_at + threadIdx.x < capacity)
		out[row_at + threadIdx.x] = (uint8_t) (threadIdx.x < 2u ? 2u : threadIdx.x == 2u ? width >> 8 : width & 255u);
	byte_writer writer = {out, row_at + 4u, capacity};
	for (uint32_t q = 0; q != plane; ++q) writer.base += plane_sizes[4u * y + q];
	rgbe_loader load = {rgbe + (uint64_t) y * width};
	code_row(width, load, writer, staged);
}

// widths that are not run-length coded: lane t writes byte t of the header and the quadruple of pixel t
__global__ void __launch_bounds__(256) k_hdr_raw(hdr_source source, uint32_t width, uint64_t pixel_count, const uint8_t* header, uint32_t header_size,
                                                uint8_t* out, uint64_t capacity, uint64_t* size_word) {
	uint64_t i = (uint64_t) blockIdx.x * 256u + threadIdx.x;
	if (i < header_size && i < capacity) out[i] = header[i];
	if (i == 0u) *size_word = header_size + 4ull * pixel_count;
	if (i >= pixel_count) return;
	uint32_t rgbe = load_rgbe(source, (uint32_t) (i % width), (uint32_t) (i / width));
	uint64_t at = header_size + 4ull * i;
#pragma unroll
	for (uint32_t c = 0; c != 4u; ++c)
		if (at + c < capacity) out[at + c] = (uint8_t) (rgbe >> (8u * c));
}

// ---- the encoder ------------------------------------------------------------------------------------------------------

// the scratch memory of a slot besides what output_slots.h keeps
struct hdr_slot {
	uint32_t *rgbe, *plane_sizes;
	uint64_t *row_sizes, *row_offsets;
};

struct hdr_state {
	// (what its slots share: the header)
	output_slots out;
	hdr_slot slots[kMaxOutputSlots];
};

output_slots* slots_of(const hdr_encoder_t* encoder) { return encoder && encoder->state ? &((hdr_state*) encoder->state)->out : NULL; }

bool run_length_coded(uint32_t width) { return width >= 8 && width < 32768; }

// (raw widths need the record alone)
void lay_out_slot(output_carver& carve, void* hdr_encoder_pointer, uint32_t slot_index) {
	const hdr_encoder_t* encoder = (const hdr_encoder_t*) hdr_encoder_pointer;
	hdr_slot& slot = ((hdr_state*) encoder->state)->slots[slot_index];
	size_t pixels = encoder->run_length_coded ? (size_t) encoder->width * encoder->height : 0, rows = encoder->run_length_coded ? encoder->height : 0;
	carve.take(slot.rgbe, pixels);
	carve.take(slot.plane_sizes, rows * 4);
	carve.take(slot.row_sizes, rows + 1);
	carve.take(slot.row_offsets, rows + 1);
}

int enqueue_encode(hdr_encoder_t* encoder, uint32_t slot_index, const void* device_pixels, uint32_t channel_count, uint64_t row_stride_bytes, VkBool32 through_half,
                   uint8_t* out, uint64_t capacity, uint64_t* size_word, bool copy_out, void* stream_or_null) {
	hdr_state* state = (hdr_state*) encoder->state;
	if (!state || !device_pixels || (channel_count != 3 && channel_count != 4) || (uintptr_t) device_pixels % 4 != 0) {
		printf("An HDR encode needs an encoder and device pixels of 3 or 4 floats.\n");
		return 1;
	}
	uint64_t row_bytes = (uint64_t) encoder->width * channel_count * sizeof(float);
	if (row_stride_bytes == 0) row_stride_bytes = row_bytes;
	if (row_stride_bytes < row_bytes || row_stride_bytes % 4 != 0) {
		printf("A row stride of %llu bytes is less than a row of %u pixels of %u floats, or no multiple of four.\n", (unsigned long long) row_stride_bytes, encoder->width, channel_count);
		return 1;
	}
	hipStream_t stream;
	if (begin_output_enqueue(&state->out, slot_index, stream_or_null, &stream)) return 1;
	const hdr_slot& slot = state->slots[slot_index];
	const uint8_t* header = state->out.shared;
	uint32_t width = encoder->width, height = encoder->height;
	hdr_source source = {(const uint8_t*) device_pixels, row_stride_bytes, channel_count, through_half ? 1u : 0u,
		(channel_count == 4 && (uintptr_t) device_pixels % 16 == 0 && row_stride_bytes % 16 == 0) ? 1u : 0u};
	if (encoder->run_length_coded) {
		k_hdr_row_sizes<<<height, 256, 0, stream>>>(source, width, height, slot.rgbe, slot.plane_sizes, slot.row_sizes);
		size_t scan_bytes = state->out.scan_bytes;
		if (hip_failed(hipcub::DeviceScan::ExclusiveSum(state->out.slots[slot_index].scan_storage, scan_bytes, slot.row_sizes, slot.row_offsets, (int) (height + 1), stream), "summing the sizes of the rows")) return 1;
		k_hdr_write_rows<<<height, 256, 0, stream>>>(slot.rgbe, width, height, slot.plane_sizes, slot.row_offsets, header, encoder->header_size, out, capacity, size_word);
	}
	else {
		uint64_t pixel_count = (uint64_t) width * height;
		k_hdr_raw<<<block_count(pixel_count > encoder->header_size ? pixel_count : encoder->header_size, 256), 256, 0, stream>>>(source, width, pixel_count, header, encoder->header_size, out, capacity, size_word);
	}
	return finish_output_enqueue(&state->out, slot_index, stream, copy_out ? 256 : 0);
}

}  // namespace

extern "C" uint32_t get_hdr_chunk_size(void) { return kChunk; }

extern "C" uint32_t get_hdr_segment_size(void) { return kSegment; }

extern "C" uint32_t get_hdr_header(char header[VKR_HDR_MAX_HEADER_SIZE], uint32_t width, uint32_t height) {
	if (!valid_output_extent(width, height)) return 0;
	return (uint32_t) snprintf(header, VKR_HDR_MAX_HEADER_SIZE, "#?RADIANCE\n# Written by stb_image_write.h\nFORMAT=32-bit_rle_rgbe\nEXPOSURE=          1.0000000000000\n\n-Y %d +X %d\n", (int) height, (int) width);
}

extern "C" uint64_t get_hdr_capacity(uint32_t width, uint32_t height) {
	char header[VKR_HDR_MAX_HEADER_SIZE];
	uint64_t header_size = get_hdr_header(header, width, height);
	if (!header_size) return 0;
	if (!run_length_coded(width)) return header_size + 4ull * width * height;
	return header_size + (uint64_t) height * (4ull + 4ull * (width + (width + 127u) / 128u));
}

extern "C" int write_hdr_file(const char* path, const uint8_t* bytes, uint64_t size) { return vkr_write_file(path, bytes, size); }

extern "C" void destroy_hdr_encoder(hdr_encoder_t* encoder) {
	hdr_state* state = encoder ? (hdr_state*) encoder->state : NULL;
	if (state) {
		destroy_output_slots(&state->out);
		free(state);
	}
	if (encoder) memset(encoder, 0, sizeof(*encoder));
}

extern "C" int create_hdr_encoder(hdr_encoder_t* encoder, const device_t* device, uint32_t width, uint32_t height, uint32_t slot_count) {
	memset(encoder, 0, sizeof(*encoder));
	if (check_output_arguments("HDR", device, width, height, slot_count)) return 1;
	hdr_state* state = (hdr_state*) calloc(1, sizeof(hdr_state));
	if (!state) {
		printf("Out of memory creating an HDR encoder.\n");
		return 1;
	}
	char header[VKR_HDR_MAX_HEADER_SIZE];
	encoder->width = width; encoder->height = height;
	encoder->slot_count = slot_count;
	encoder->header_size = get_hdr_header(header, width, height);
	encoder->run_length_coded = run_length_coded(width);
	encoder->capacity = get_hdr_capacity(width, height);
	encoder->state = state;
	size_t scan_bytes = 0;
	int failed = (encoder->run_length_coded && hip_failed(hipcub::DeviceScan::ExclusiveSum(NULL, scan_bytes, (uint64_t*) NULL, (uint64_t*) NULL, (int) (height + 1), (hipStream_t) device->stream), "sizing the sum of the row sizes"))
		|| create_output_slots(&state->out, "HDR", device, slot_count, encoder->capacity, 0, scan_bytes, header, VKR_HDR_MAX_HEADER_SIZE, lay_out_slot, encoder);
	if (failed) destroy_hdr_encoder(encoder);
	return failed;
}

extern "C" int begin_hdr_encode(hdr_encoder_t* encoder, uint32_t slot, const void* device_pixels, uint32_t channel_count, uint64_t row_stride_bytes, VkBool32 through_half, void* stream) {
	if (check_output_slot(slots_of(encoder), slot)) return 1;
	uint8_t* record = slots_of(encoder)->slots[slot].record;
	return enqueue_encode(encoder, slot, device_pixels, channel_count, row_stride_bytes, through_half, record + 16, encoder->capacity, (uint64_t*) record, true, stream);
}

extern "C" int end_hdr_encode(hdr_encoder_t* encoder, uint32_t slot, const uint8_t** bytes, uint64_t* size) { return end_output_encode(slots_of(encoder), slot, bytes, size); }

extern "C" int encode_hdr(hdr_encoder_t* encoder, const void* device_pixels, uint32_t channel_count, uint64_t row_stride_bytes, VkBool32 through_half, const uint8_t** bytes, uint64_t* size) {
	return begin_hdr_encode(encoder, 0, device_pixels, channel_count, row_stride_bytes, through_half, NULL) || end_hdr_encode(encoder, 0, bytes, size);
}

extern "C" int encode_hdr_on_device(hdr_encoder_t* encoder, const void* device_pixels, uint32_t channel_count, uint64_t row_stride_bytes, VkBool32 through_half,
                                    void* device_out, uint64_t capacity, uint64_t* device_size_word, void* stream) {
	if (check_output_slot(slots_of(encoder), 0)) return 1;
	if (!device_out || !device_size_word) {
		printf("encode_hdr_on_device() needs device memory for the file and for its size.\n");
		return 1;
	}
	return enqueue_encode(encoder, 0, device_pixels, channel_count, row_stride_bytes, through_half, (uint8_t*) device_out, capacity, device_size_word, false, stream);
}
