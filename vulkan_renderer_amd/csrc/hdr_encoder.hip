// Frames as Radiance RGBE files on the device (include/vkr_hdr.h states the rule).  One encode is a chain of kernels on
// the caller's stream, without a host wait in between.  For run-length coded widths, one workgroup per row:
//   k_hdr_row_sizes      floats -> RGBE dwords (kept for the second pass), the coded size of the row's four planes
//   hipcub exclusive sum, 64 bit, over the rows
//   k_hdr_write_rows     header, scanline headers, the coded planes at their offsets, size word
// for the other widths k_hdr_raw alone: header, RGBE quadruples, size word.  Then
//   k_hdr_copy_out       the size record and that many bytes into the slot's pinned staging memory
// The coding exists once, code_row<Load, Sink>: the first pass runs it with a sink that drops the bytes and keeps the
// positions, the second with one that stores them, so that sizes and bytes cannot disagree.
// This unit is compiled without contraction whatever the arithmetic mode of the pass: the bytes are the interface.
#include "vkr_hdr.h"
#include "host/vkr_internal.h"
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <hipcub/hipcub.hpp>
#include <float.h>

namespace {

constexpr uint32_t kChunk = VKR_HDR_CHUNK;
constexpr uint32_t kSegment = VKR_HDR_SEGMENT;
constexpr uint32_t kMaxSlots = VKR_MAX_FRAMES_IN_FLIGHT + 1;
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

// record: the size in its first 8 of 16 bytes, then the file.  Sixteen bytes per lane into host memory.
__global__ void __launch_bounds__(256) k_hdr_copy_out(const uint4* record, uint4* staging, uint64_t capacity_units) {
	uint64_t units = min(1 + (*(const uint64_t*) record + 15) / 16, capacity_units);
	for (uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x; i < units; i += (uint64_t) gridDim.x * 256) staging[i] = record[i];
}

// ---- the encoder ------------------------------------------------------------------------------------------------------

struct hdr_slot {
	uint32_t *rgbe, *plane_sizes;
	uint64_t *row_sizes, *row_offsets;
	uint8_t* record;
	void* scan_storage;
	// pinned host memory with the layout of record, and its address on the device
	uint8_t *staging, *staging_device;
	hipEvent_t done;
	bool begun;
};

struct hdr_state {
	void* stream;
	uint8_t* header;
	uint64_t record_units;
	size_t scan_bytes;
	void* scratch;
	hdr_slot slots[kMaxSlots];
};

bool valid_extent(uint32_t width, uint32_t height) { return width != 0 && height != 0 && width <= 65535 && height <= 65535; }

bool run_length_coded(uint32_t width) { return width >= 8 && width < 32768; }

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
	hipStream_t stream = (hipStream_t) (stream_or_null ? stream_or_null : state->stream);
	hdr_slot& slot = state->slots[slot_index];
	uint32_t width = encoder->width, height = encoder->height;
	// the scratch memory of the slot is free once its previous encode is through
	if (hip_failed(hipStreamWaitEvent(stream, slot.done, 0), "ordering an HDR encode behind the slot's previous one")) return 1;
	hdr_source source = {(const uint8_t*) device_pixels, row_stride_bytes, channel_count, through_half ? 1u : 0u,
		(channel_count == 4 && (uintptr_t) device_pixels % 16 == 0 && row_stride_bytes % 16 == 0) ? 1u : 0u};
	if (encoder->run_length_coded) {
		k_hdr_row_sizes<<<height, 256, 0, stream>>>(source, width, height, slot.rgbe, slot.plane_sizes, slot.row_sizes);
		size_t scan_bytes = state->scan_bytes;
		if (hip_failed(hipcub::DeviceScan::ExclusiveSum(slot.scan_storage, scan_bytes, slot.row_sizes, slot.row_offsets, (int) (height + 1), stream), "summing the sizes of the rows")) return 1;
		k_hdr_write_rows<<<height, 256, 0, stream>>>(slot.rgbe, width, height, slot.plane_sizes, slot.row_offsets, state->header, encoder->header_size, out, capacity, size_word);
	}
	else {
		uint64_t pixel_count = (uint64_t) width * height;
		k_hdr_raw<<<block_count(pixel_count > encoder->header_size ? pixel_count : encoder->header_size, 256), 256, 0, stream>>>(source, width, pixel_count, state->header, encoder->header_size, out, capacity, size_word);
	}
	if (copy_out) k_hdr_copy_out<<<256, 256, 0, stream>>>((const uint4*) slot.record, (uint4*) slot.staging_device, state->record_units);
	if (hip_failed(hipGetLastError(), "encoding an HDR file")) return 1;
	return hip_failed(hipEventRecord(slot.done, stream), "recording the end of an HDR encode");
}

int check_slot(const hdr_encoder_t* encoder, uint32_t slot) {
	if (encoder && encoder->state && slot < encoder->slot_count) return 0;
	printf("Slot %u is not a slot of this HDR encoder.\n", slot);
	return 1;
}

}  // namespace

extern "C" uint32_t get_hdr_chunk_size(void) { return kChunk; }

extern "C" uint32_t get_hdr_segment_size(void) { return kSegment; }

extern "C" uint32_t get_hdr_header(char header[VKR_HDR_MAX_HEADER_SIZE], uint32_t width, uint32_t height) {
	if (!valid_extent(width, height)) return 0;
	return (uint32_t) snprintf(header, VKR_HDR_MAX_HEADER_SIZE, "#?RADIANCE\n# Written by stb_image_write.h\nFORMAT=32-bit_rle_rgbe\nEXPOSURE=          1.0000000000000\n\n-Y %d +X %d\n", (int) height, (int) width);
}

extern "C" uint64_t get_hdr_capacity(uint32_t width, uint32_t height) {
	char header[VKR_HDR_MAX_HEADER_SIZE];
	uint64_t header_size = get_hdr_header(header, width, height);
	if (!header_size) return 0;
	if (!run_length_coded(width)) return header_size + 4ull * width * height;
	return header_size + (uint64_t) height * (4ull + 4ull * (width + (width + 127u) / 128u));
}

extern "C" int write_hdr_file(const char* path, const uint8_t* bytes, uint64_t size) {
	FILE* file = (path && bytes) ? fopen(path, "wb") : NULL;
	if (!file) {
		printf("Failed to open %s for writing.\n", path ? path : "(null)");
		return 1;
	}
	int failed = fwrite(bytes, 1, size, file) != size;
	failed |= fclose(file) != 0;
	if (failed) printf("Failed to write %s.\n", path);
	return failed;
}

extern "C" void destroy_hdr_encoder(hdr_encoder_t* encoder) {
	hdr_state* state = encoder ? (hdr_state*) encoder->state : NULL;
	if (state) {
		for (uint32_t i = 0; i != kMaxSlots; ++i) {
			hdr_slot& slot = state->slots[i];
			if (slot.done) {
				(void) hipEventSynchronize(slot.done);
				(void) hipEventDestroy(slot.done);
			}
			if (slot.staging) (void) hipHostFree(slot.staging);
		}
		if (state->scratch) (void) hipFree(state->scratch);
		free(state);
	}
	if (encoder) memset(encoder, 0, sizeof(*encoder));
}

extern "C" int create_hdr_encoder(hdr_encoder_t* encoder, const device_t* device, uint32_t width, uint32_t height, uint32_t slot_count) {
	memset(encoder, 0, sizeof(*encoder));
	if (!device) {
		printf("The HDR encoder runs on the device: it has no host build.\n");
		return 1;
	}
	if (!valid_extent(width, height)) {
		printf("An HDR file of this encoder is between 1 x 1 and 65535 x 65535 pixels, not %u x %u.\n", width, height);
		return 1;
	}
	if (slot_count == 0 || slot_count > kMaxSlots) {
		printf("An HDR encoder has 1 to %u slots, not %u.\n", kMaxSlots, slot_count);
		return 1;
	}
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
	state->stream = device->stream;
	state->record_units = 1 + (encoder->capacity + 15) / 16;
	int failed = 0;
	if (encoder->run_length_coded)
		failed = hip_failed(hipcub::DeviceScan::ExclusiveSum(NULL, state->scan_bytes, (uint64_t*) NULL, (uint64_t*) NULL, (int) (height + 1), (hipStream_t) device->stream), "sizing the sum of the row sizes");
	// one allocation: the header, then the scratch memory of every slot (raw widths need the record alone)
	size_t pixels = encoder->run_length_coded ? (size_t) width * height : 0, rows = encoder->run_length_coded ? height : 0;
	size_t total = 0, header_at = vkr_carve(&total, VKR_HDR_MAX_HEADER_SIZE), at[kMaxSlots][6];
	for (uint32_t i = 0; i != slot_count; ++i) {
		at[i][0] = vkr_carve(&total, pixels * sizeof(uint32_t));
		at[i][1] = vkr_carve(&total, rows * 4 * sizeof(uint32_t));
		at[i][2] = vkr_carve(&total, (rows + 1) * sizeof(uint64_t));
		at[i][3] = vkr_carve(&total, (rows + 1) * sizeof(uint64_t));
		at[i][4] = vkr_carve(&total, state->record_units * 16);
		at[i][5] = vkr_carve(&total, state->scan_bytes ? state->scan_bytes : 1);
	}
	failed = failed || hip_failed(hipMalloc(&state->scratch, total), "allocating the scratch memory of an HDR encoder");
	if (!failed) {
		uint8_t* base = (uint8_t*) state->scratch;
		state->header = base + header_at;
		// k_hdr_copy_out copies whole 16-byte units, the rest of the size record and the tail behind the file included: no stale device memory reaches the host
		failed = hip_failed(hipMemsetAsync(state->scratch, 0, total, (hipStream_t) device->stream), "clearing the scratch memory of an HDR encoder")
			|| hip_failed(hipStreamSynchronize((hipStream_t) device->stream), "clearing the scratch memory of an HDR encoder")
			|| hip_failed(hipMemcpy(state->header, header, VKR_HDR_MAX_HEADER_SIZE, hipMemcpyHostToDevice), "uploading the header of an HDR file");
		for (uint32_t i = 0; i != slot_count && !failed; ++i) {
			hdr_slot& slot = state->slots[i];
			slot.rgbe = (uint32_t*) (base + at[i][0]);
			slot.plane_sizes = (uint32_t*) (base + at[i][1]);
			slot.row_sizes = (uint64_t*) (base + at[i][2]);
			slot.row_offsets = (uint64_t*) (base + at[i][3]);
			slot.record = base + at[i][4];
			slot.scan_storage = base + at[i][5];
			failed = hip_failed(hipHostMalloc((void**) &slot.staging, state->record_units * 16, hipHostMallocDefault), "allocating the pinned staging memory of an HDR encoder")
				|| hip_failed(hipHostGetDevicePointer((void**) &slot.staging_device, slot.staging, 0), "mapping the staging memory of an HDR encoder")
				|| hip_failed(hipEventCreateWithFlags(&slot.done, hipEventDisableTiming), "creating the event of an HDR slot");
		}
	}
	if (failed) destroy_hdr_encoder(encoder);
	return failed;
}

extern "C" int begin_hdr_encode(hdr_encoder_t* encoder, uint32_t slot, const void* device_pixels, uint32_t channel_count, uint64_t row_stride_bytes, VkBool32 through_half, void* stream) {
	if (check_slot(encoder, slot)) return 1;
	hdr_slot& target = ((hdr_state*) encoder->state)->slots[slot];
	if (enqueue_encode(encoder, slot, device_pixels, channel_count, row_stride_bytes, through_half, target.record + 16, encoder->capacity, (uint64_t*) target.record, true, stream)) return 1;
	target.begun = true;
	return 0;
}

extern "C" int end_hdr_encode(hdr_encoder_t* encoder, uint32_t slot, const uint8_t** bytes, uint64_t* size) {
	if (check_slot(encoder, slot)) return 1;
	hdr_slot& source = ((hdr_state*) encoder->state)->slots[slot];
	if (!source.begun) {
		printf("end_hdr_encode() without begin_hdr_encode() on slot %u.\n", slot);
		return 1;
	}
	if (hip_failed(hipEventSynchronize(source.done), "waiting for an HDR encode")) return 1;
	*size = *(const uint64_t*) source.staging;
	*bytes = source.staging + 16;
	return 0;
}

extern "C" int encode_hdr(hdr_encoder_t* encoder, const void* device_pixels, uint32_t channel_count, uint64_t row_stride_bytes, VkBool32 through_half, const uint8_t** bytes, uint64_t* size) {
	return begin_hdr_encode(encoder, 0, device_pixels, channel_count, row_stride_bytes, through_half, NULL) || end_hdr_encode(encoder, 0, bytes, size);
}

extern "C" int encode_hdr_on_device(hdr_encoder_t* encoder, const void* device_pixels, uint32_t channel_count, uint64_t row_stride_bytes, VkBool32 through_half,
                                    void* device_out, uint64_t capacity, uint64_t* device_size_word, void* stream) {
	if (check_slot(encoder, 0)) return 1;
	if (!device_out || !device_size_word) {
		printf("encode_hdr_on_device() needs device memory for the file and for its size.\n");
		return 1;
	}
	return enqueue_encode(encoder, 0, device_pixels, channel_count, row_stride_bytes, through_half, (uint8_t*) device_out, capacity, device_size_word, false, stream);
}
