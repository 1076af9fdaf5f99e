// Frames as PNG files on the device (include/vkr_png.h states the rule).  One encode is a chain of kernels on the
// caller's stream, without a host wait in between:
//   k_png_filter      pixels -> the filtered stream F: one workgroup per row, the five costs, then the chosen residuals
//   k_png_parse       one workgroup per unit of 4096 bytes: equality bits for the three distances by ballots, match
//                     lengths by bit scans, the greedy chain by pointer jumping in LDS, tokens, the segment's counts
//                     (LDS first, then integer atomics), the unit's Adler sums
//   k_png_codes       one workgroup per segment: three Huffman codes, fixed or dynamic, the block header
//   hipcub exclusive sum, 64 bit, over the chunk sizes
//   k_png_unit_bits   the bits of every unit's tokens in the chosen code; hipcub exclusive sum, 64 bit, over them
//   k_png_pack        the bits of tokens, headers, ends of block and stored blocks, by atomic OR into the cleared file
//   k_png_adler       the Adler-32 from the units' sums
//   k_png_frame       one workgroup per segment: chunk length, type and CRC-32 (slices per lane, combined by products
//                     with x^(8 n) mod P), signature, IHDR, IEND, size word
//   k_copy_record_out (output_slots.hip) the size record and that many bytes into the slot's pinned staging memory
// The probe of the header enters behind the filter with a stream of the caller's.
#include "vkr_png.h"
#include "output_slots.h"
#include <hipcub/hipcub.hpp>

namespace {

constexpr uint32_t kUnit = VKR_PNG_UNIT;
constexpr uint32_t kLiterals = 286, kDistances = 30, kSymbols = kLiterals + kDistances, kMetaSymbols = 19;
constexpr uint32_t kEndOfBlock = 256, kMaxMatch = 258;
// words of block header per segment: 3 + 14 + 57 + 316 * 7 bits at most
constexpr uint32_t kHeaderWords = 72;
// positions of a unit per lane of a workgroup of 256
constexpr uint32_t kPerLane = kUnit / 256;
constexpr uint32_t kMaxProbeRowLength = 262144;
static_assert(kUnit == 4096 && kPerLane == 16, "a unit is sixteen positions for each of 256 lanes, 64 ballots of 64");

// the stream and its segments, the same for every kernel of an encode
struct png_shape {
	uint32_t row_length, rows, rows_per_segment, segment_count, units_per_row, unit_count;
	// whether the row length is a candidate distance; its distance symbol, the count of its extra bits and their value
	uint32_t row_candidate, row_symbol, row_extra_bits, row_extra;
	uint64_t stream_size;
};

struct png_segment {
	// bits of BFINAL, BTYPE and the dynamic header; bits of the tokens and the end of block in the chosen code
	uint32_t header_bits, token_bits;
	// the reversed code of the end of block | its length << 16
	uint32_t end_of_block;
	uint32_t dynamic;
};

struct png_source {
	const uint8_t* pixels;
	uint64_t stride;
	uint32_t channels;
};

// ---- filter -----------------------------------------------------------------------------------------------------------

__device__ inline int paeth(int a, int b, int c) {
	int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
	return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ inline int predict(uint32_t filter, int a, int b, int c) {
	return filter == 0 ? 0 : filter == 1 ? a : filter == 2 ? b : filter == 3 ? (a + b) >> 1 : paeth(a, b, c);
}

__global__ void __launch_bounds__(256) k_png_filter(png_source source, uint32_t width, uint8_t* filtered) {
	__shared__ uint32_t costs[5];
	const uint32_t y = blockIdx.x, count = 3u * width;
	const uint8_t* row = source.pixels + (uint64_t) y * source.stride;
	const uint8_t* above = y ? row - source.stride : nullptr;
	uint8_t* out = filtered + (uint64_t) y * (count + 1u);
	if (threadIdx.x < 5u) costs[threadIdx.x] = 0u;
	__syncthreads();
	uint32_t cost[5] = {0u, 0u, 0u, 0u, 0u};
	for (uint32_t x = threadIdx.x; x < count; x += 256u) {
		uint32_t pixel = x / 3u, at = pixel * source.channels + (x - 3u * pixel);
		int value = row[at], a = pixel ? row[at - source.channels] : 0, b = above ? above[at] : 0, c = (above && pixel) ? above[at - source.channels] : 0;
#pragma unroll
		for (uint32_t filter = 0; filter != 5u; ++filter) cost[filter] += (uint32_t) abs((int) (int8_t) (uint8_t) (value - predict(filter, a, b, c)));
	}
#pragma unroll
	for (uint32_t filter = 0; filter != 5u; ++filter) atomicAdd(&costs[filter], cost[filter]);
	__syncthreads();
	// a later filter wins only if it is strictly cheaper
	uint32_t best = 0;
	for (uint32_t filter = 1; filter != 5u; ++filter)
		if (costs[filter] < costs[best]) best = filter;
	if (threadIdx.x == 0u) out[0] = (uint8_t) best;
	for (uint32_t x = threadIdx.x; x < count; x += 256u) {
		uint32_t pixel = x / 3u, at = pixel * source.channels + (x - 3u * pixel);
		int value = row[at], a = pixel ? row[at - source.channels] : 0, b = above ? above[at] : 0, c = (above && pixel) ? above[at - source.channels] : 0;
		out[1u + x] = (uint8_t) (value - predict(best, a, b, c));
	}
}

// ---- tokens -----------------------------------------------------------------------------------------------------------

// The consecutive set bits from bit p on, at most kMaxMatch.  The word behind the unit's last is zero.
__device__ inline uint32_t run_length(const uint64_t* equal, uint32_t p) {
	uint32_t word = p >> 6, bit = p & 63u;
	uint64_t zeros = ~equal[word] >> bit;
	if (zeros) return min((uint32_t) __ffsll((long long) zeros) - 1u, kMaxMatch);
	uint32_t length = 64u - bit;
	while (length < kMaxMatch) {
		zeros = ~equal[++word];
		if (zeros) {
			length += (uint32_t) __ffsll((long long) zeros) - 1u;
			break;
		}
		length += 64u;
	}
	return min(length, kMaxMatch);
}

// index into the 29 length symbols, the count of extra bits and their value
__device__ inline void length_symbol(uint32_t length, uint32_t& index, uint32_t& extra_bits, uint32_t& extra) {
	if (length < 11u || length == kMaxMatch) {
		index = length == kMaxMatch ? 28u : length - 3u;
		extra_bits = extra = 0u;
		return;
	}
	uint32_t m = length - 3u;
	extra_bits = 29u - (uint32_t) __clz((int) m);
	index = 4u * extra_bits + 4u + ((m >> extra_bits) & 3u);
	extra = m & ((1u << extra_bits) - 1u);
}

__device__ inline uint32_t distance_symbol_of(uint32_t selector, const png_shape& shape) { return selector == 0u ? 0u : selector == 1u ? 2u : shape.row_symbol; }

// A token is 0 where none starts, 1 for a literal, length | selector << 9 for a match (selector 0, 1, 2: distance 1, 3, L).
__global__ void __launch_bounds__(256) k_png_parse(png_shape shape, const uint8_t* filtered, uint16_t* tokens, uint32_t* histograms, uint32_t* unit_sums) {
	// bytes[3 + i] is byte i of the unit, bytes[0 ... 2] the three in front of it
	__shared__ uint8_t bytes[kUnit + 4];
	__shared__ uint64_t equal[3][kUnit / 64 + 1];
	__shared__ uint16_t token[kUnit];
	__shared__ uint16_t jump[kUnit + 2];
	__shared__ uint8_t mark[kUnit];
	__shared__ uint32_t counts[kSymbols];
	__shared__ uint32_t sums[2];
	const uint32_t unit = blockIdx.x, row = unit / shape.units_per_row, first = (unit % shape.units_per_row) * kUnit;
	const uint32_t count = min(kUnit, shape.row_length - first), lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint64_t base = (uint64_t) row * shape.row_length + first;
	for (uint32_t i = threadIdx.x; i < count + 3u; i += 256u) bytes[i] = base + i >= 3u ? filtered[base + i - 3u] : (uint8_t) 0;
	for (uint32_t i = threadIdx.x; i < kUnit; i += 256u) mark[i] = 0;
	for (uint32_t i = threadIdx.x; i < kSymbols; i += 256u) counts[i] = 0u;
	if (threadIdx.x < 2u) sums[threadIdx.x] = 0u;
	if (threadIdx.x < 3u) {
		for (uint32_t w = 0; w != kUnit / 64 + 1; ++w) equal[threadIdx.x][w] = 0ull;
	}
	__syncthreads();
	const uint32_t rounds = (count + 255u) / 256u;
	uint32_t sum = 0, weighted = 0;
	for (uint32_t c = 0; c != rounds; ++c) {
		uint32_t p = c * 256u + threadIdx.x;
		bool valid = p < count;
		uint32_t value = valid ? bytes[3u + p] : 0u;
		uint64_t at = base + p;
		bool e1 = valid && at >= 1u && value == bytes[2u + p];
		bool e3 = valid && at >= 3u && value == bytes[p];
		bool el = valid && shape.row_candidate && row >= 1u && value == filtered[at - shape.row_length];
		uint64_t b1 = __ballot(e1), b3 = __ballot(e3), bl = __ballot(el);
		if (lane == 0u) {
			equal[0][4u * c + wave] = b1;
			equal[1][4u * c + wave] = b3;
			equal[2][4u * c + wave] = bl;
		}
		sum += value;
		weighted += valid ? (count - p) * value : 0u;
	}
	atomicAdd(&sums[0], sum);
	atomicAdd(&sums[1], weighted);
	__syncthreads();
	for (uint32_t c = 0; c != rounds; ++c) {
		uint32_t p = c * 256u + threadIdx.x;
		if (p < count) {
			uint32_t best = run_length(equal[0], p), selector = 0u, other = run_length(equal[1], p);
			if (other > best) { best = other; selector = 1u; }
			other = run_length(equal[2], p);
			if (other > best) { best = other; selector = 2u; }
			bool match = best >= 3u;
			token[p] = (uint16_t) (match ? best | (selector << 9) : 1u);
			jump[p] = (uint16_t) (p + (match ? best : 1u));
		}
	}
	if (threadIdx.x == 0u) {
		jump[count] = (uint16_t) count;
		mark[0] = 1;
	}
	__syncthreads();
	// after k rounds the positions less than 2^k tokens behind the unit's start are marked and jump is 2^k tokens wide
	for (uint32_t span = 1; span < count; span <<= 1) {
		uint16_t to[kPerLane], further[kPerLane];
		uint8_t marked[kPerLane];
#pragma unroll
		for (uint32_t c = 0; c != kPerLane; ++c) {
			uint32_t p = c * 256u + threadIdx.x;
			if (p < count) {
				to[c] = jump[p];
				further[c] = jump[to[c]];
				marked[c] = mark[p];
			}
		}
		__syncthreads();
#pragma unroll
		for (uint32_t c = 0; c != kPerLane; ++c) {
			uint32_t p = c * 256u + threadIdx.x;
			if (p < count) {
				if (marked[c] && to[c] < count) mark[to[c]] = 1;
				jump[p] = further[c];
			}
		}
		__syncthreads();
	}
	for (uint32_t c = 0; c != rounds; ++c) {
		uint32_t p = c * 256u + threadIdx.x;
		if (p < count) {
			uint32_t t = mark[p] ? token[p] : 0u;
			tokens[base + p] = (uint16_t) t;
			if (t == 1u) atomicAdd(&counts[bytes[3u + p]], 1u);
			else if (t) {
				uint32_t index, extra_bits, extra;
				length_symbol(t & 511u, index, extra_bits, extra);
				atomicAdd(&counts[257u + index], 1u);
				atomicAdd(&counts[kLiterals + distance_symbol_of(t >> 9, shape)], 1u);
			}
		}
	}
	__syncthreads();
	uint32_t* histogram = histograms + (uint64_t) (row / shape.rows_per_segment) * kSymbols;
	for (uint32_t i = threadIdx.x; i < kSymbols; i += 256u)
		if (counts[i]) atomicAdd(&histogram[i], counts[i]);
	if (threadIdx.x < 2u) unit_sums[2ull * unit + threadIdx.x] = sums[threadIdx.x];
}

// ---- codes ------------------------------------------------------------------------------------------------------------

struct code_scratch {
	uint32_t symbol[kLiterals], weight[kLiterals], node[kLiterals];
	uint16_t leaf_parent[kLiterals], node_parent[kLiterals];
	uint32_t used, longest;
	uint32_t of_length[16], next[16];
};

// CODES of the rule, steps 1 to 3, by the whole workgroup.  counts (LDS) end up padded and halved.
__device__ void build_lengths(uint32_t* counts, uint32_t symbol_count, uint32_t limit, uint32_t* lengths, code_scratch& w) {
	if (threadIdx.x == 0u) w.used = 0u;
	__syncthreads();
	for (uint32_t s = threadIdx.x; s < symbol_count; s += 256u)
		if (counts[s]) atomicAdd(&w.used, 1u);
	__syncthreads();
	if (threadIdx.x == 0u) {
		uint32_t used = w.used;
		for (uint32_t s = 0; used < 2u; ++s)
			if (!counts[s]) {
				counts[s] = 1u;
				++used;
			}
	}
	__syncthreads();
	for (;;) {
		if (threadIdx.x == 0u) w.used = w.longest = 0u;
		__syncthreads();
		// the place of every symbol with a count among them, by (count, symbol)
		for (uint32_t s = threadIdx.x; s < symbol_count; s += 256u) {
			lengths[s] = 0u;
			uint32_t c = counts[s];
			if (!c) continue;
			uint32_t rank = 0;
			for (uint32_t q = 0; q != symbol_count; ++q) {
				uint32_t other = counts[q];
				rank += (other && (other < c || (other == c && q < s))) ? 1u : 0u;
			}
			w.symbol[rank] = s;
			w.weight[rank] = c;
			atomicAdd(&w.used, 1u);
		}
		__syncthreads();
		if (threadIdx.x == 0u) {
			// two queues: the leaves in their order, the joined nodes in the order of their making
			// The weights of the next two leaves (i, i + 1) and joined nodes (h, h + 1) are kept in registers, `none` where
			// there is no such node yet, so that a pick never waits for the load that the pick before it caused.
			const uint32_t m = w.used, none = 0xFFFFFFFFu;
			uint32_t i = 0, h = 0;
			uint32_t leaf0 = w.weight[0], leaf1 = m > 1u ? w.weight[1] : none, node0 = none, node1 = none;
			for (uint32_t k = 0; k + 1u < m; ++k) {
				uint32_t total = 0;
				for (uint32_t pick = 0; pick != 2u; ++pick) {
					if (i < m && (h >= k || leaf0 <= node0)) {
						total += leaf0;
						w.leaf_parent[i++] = (uint16_t) k;
						leaf0 = leaf1;
						leaf1 = i + 1u < m ? w.weight[i + 1u] : none;
					}
					else {
						total += node0;
						w.node_parent[h++] = (uint16_t) k;
						node0 = node1;
						node1 = h + 1u < k ? w.node[h + 1u] : none;
					}
				}
				w.node[k] = total;
				if (h == k) node0 = total;
				else if (h + 1u == k) node1 = total;
			}
		}
		__syncthreads();
		// a leaf's depth: the joins from it up to the last one, the root (a walk per lane; the joins were one lane's chain)
		for (uint32_t leaf = threadIdx.x; leaf < w.used; leaf += 256u) {
			uint32_t length = 1u;
			for (uint32_t node = w.leaf_parent[leaf]; node + 2u != w.used; node = w.node_parent[node]) ++length;
			lengths[w.symbol[leaf]] = length;
			atomicMax(&w.longest, length);
		}
		__syncthreads();
		if (w.longest <= limit) break;
		for (uint32_t s = threadIdx.x; s < symbol_count; s += 256u)
			if (counts[s]) counts[s] = (counts[s] + 1u) >> 1;
		__syncthreads();
	}
	__syncthreads();
}

// RFC 1951 3.2.2, the codes with their bits reversed: as they enter a stream that is filled from the least significant bit
__device__ void assign_codes(const uint32_t* lengths, uint32_t symbol_count, uint32_t* codes, code_scratch& w) {
	if (threadIdx.x < 16u) w.of_length[threadIdx.x] = 0u;
	__syncthreads();
	for (uint32_t s = threadIdx.x; s < symbol_count; s += 256u)
		if (lengths[s]) atomicAdd(&w.of_length[lengths[s]], 1u);
	__syncthreads();
	if (threadIdx.x == 0u) {
		uint32_t code = 0;
		for (uint32_t bits = 1; bits != 16u; ++bits) {
			code = (code + w.of_length[bits - 1u]) << 1;
			w.next[bits] = code;
		}
	}
	__syncthreads();
	for (uint32_t s = threadIdx.x; s < symbol_count; s += 256u) {
		uint32_t length = lengths[s], code = 0;
		if (length) {
			uint32_t before = 0;
			for (uint32_t q = 0; q != s; ++q) before += lengths[q] == length;
			code = __brev(w.next[length] + before) >> (32u - length);
		}
		codes[s] = code;
	}
	__syncthreads();
}

__device__ inline uint32_t extra_bits_of(uint32_t symbol) {
	if (symbol < 265u || symbol == 285u) return 0u;
	if (symbol < kLiterals) return (symbol - 261u) >> 2;
	uint32_t distance = symbol - kLiterals;
	return distance < 4u ? 0u : (distance - 2u) >> 1;
}

// the fixed code of RFC 1951 3.2.6 (the distance symbols are their own five bits)
__device__ inline void fixed_code(uint32_t symbol, uint32_t& code, uint32_t& length) {
	if (symbol < 144u) { code = 0x30u + symbol; length = 8u; }
	else if (symbol < 256u) { code = 0x190u + (symbol - 144u); length = 9u; }
	else if (symbol < 280u) { code = symbol - 256u; length = 7u; }
	else if (symbol < kLiterals) { code = 0xC0u + (symbol - 280u); length = 8u; }
	else { code = symbol - kLiterals; length = 5u; }
}

__device__ inline void put_header_bits(uint32_t* words, uint32_t& cursor, uint32_t value, uint32_t width) {
	if (!width) return;
	words[cursor >> 5] |= value << (cursor & 31u);
	if ((cursor & 31u) + width > 32u) words[(cursor >> 5) + 1u] |= value >> (32u - (cursor & 31u));
	cursor += width;
}

// tables[segment][symbol] = reversed code | length << 16 of the chosen code; headers[segment] the bits in front of the tokens;
// chunk_sizes[segment] the bytes of its IDAT chunk, chunk_sizes[segment_count] = 0: the exclusive sum ends with the total
__global__ void __launch_bounds__(256) k_png_codes(png_shape shape, const uint32_t* histograms, uint32_t* tables, uint32_t* headers, png_segment* segments, uint64_t* chunk_sizes) {
	__shared__ uint32_t counts[kSymbols], lengths[kSymbols], codes[kSymbols];
	__shared__ uint32_t meta_counts[kMetaSymbols], meta_lengths[kMetaSymbols], meta_codes[kMetaSymbols];
	__shared__ uint32_t totals[3];
	__shared__ uint32_t header[kHeaderWords];
	__shared__ uint32_t header_bits;
	__shared__ code_scratch scratch;
	typedef hipcub::BlockScan<uint32_t, 256> lane_scan;
	__shared__ typename lane_scan::TempStorage scan_storage;
	const uint32_t segment = blockIdx.x;
	const uint32_t* histogram = histograms + (uint64_t) segment * kSymbols;
	for (uint32_t i = threadIdx.x; i < kSymbols; i += 256u) counts[i] = histogram[i] + (i == kEndOfBlock ? 1u : 0u);
	if (threadIdx.x < 3u) totals[threadIdx.x] = 0u;
	if (threadIdx.x < kMetaSymbols) meta_counts[threadIdx.x] = 0u;
	if (threadIdx.x < kHeaderWords) header[threadIdx.x] = 0u;
	__syncthreads();
	build_lengths(counts, kLiterals, 15u, lengths, scratch);
	build_lengths(counts + kLiterals, kDistances, 15u, lengths + kLiterals, scratch);
	for (uint32_t i = threadIdx.x; i < kSymbols; i += 256u) atomicAdd(&meta_counts[lengths[i]], 1u);
	__syncthreads();
	build_lengths(meta_counts, kMetaSymbols, 7u, meta_lengths, scratch);
	// the bits of both codes for the counts as they were: 0 tokens dynamic, 1 tokens fixed, 2 the 316 lengths
	for (uint32_t i = threadIdx.x; i < kSymbols; i += 256u) {
		uint32_t count = histogram[i] + (i == kEndOfBlock ? 1u : 0u), extra = extra_bits_of(i), code, fixed_length;
		fixed_code(i, code, fixed_length);
		atomicAdd(&totals[0], count * (lengths[i] + extra));
		atomicAdd(&totals[1], count * (fixed_length + extra));
		atomicAdd(&totals[2], meta_lengths[lengths[i]]);
	}
	__syncthreads();
	const bool dynamic = 14u + 3u * kMetaSymbols + totals[2] + totals[0] < totals[1], last = segment + 1u == shape.segment_count;
	if (dynamic) {
		assign_codes(lengths, kLiterals, codes, scratch);
		assign_codes(lengths + kLiterals, kDistances, codes + kLiterals, scratch);
		assign_codes(meta_lengths, kMetaSymbols, meta_codes, scratch);
	}
	else {
		for (uint32_t i = threadIdx.x; i < kSymbols; i += 256u) {
			uint32_t code, length;
			fixed_code(i, code, length);
			lengths[i] = length;
			codes[i] = __brev(code) >> (32u - length);
		}
		__syncthreads();
	}
	if (threadIdx.x == 0u) {
		uint32_t cursor = 0;
		put_header_bits(header, cursor, last ? 1u : 0u, 1u);
		put_header_bits(header, cursor, dynamic ? 2u : 1u, 2u);
		if (dynamic) {
			const uint8_t order[kMetaSymbols] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
			put_header_bits(header, cursor, 29u, 5u);
			put_header_bits(header, cursor, 29u, 5u);
			put_header_bits(header, cursor, 15u, 4u);
			for (uint32_t k = 0; k != kMetaSymbols; ++k) put_header_bits(header, cursor, meta_lengths[order[k]], 3u);
		}
		header_bits = cursor + (dynamic ? totals[2] : 0u);
	}
	__syncthreads();
	if (dynamic) {
		// the 316 lengths behind the 3 + 14 + 57 bits: two symbols per lane, a sum over the lanes places them
		const uint32_t first = 2u * threadIdx.x;
		uint32_t widths[2], before;
		for (uint32_t k = 0; k != 2u; ++k) widths[k] = first + k < kSymbols ? meta_lengths[lengths[first + k]] : 0u;
		lane_scan(scan_storage).ExclusiveSum(widths[0] + widths[1], before);
		uint32_t at = 3u + 14u + 3u * kMetaSymbols + before;
		for (uint32_t k = 0; k != 2u; ++k) {
			if (!widths[k]) continue;
			uint32_t value = meta_codes[lengths[first + k]], shift = at & 31u;
			atomicOr(&header[at >> 5], value << shift);
			if (shift + widths[k] > 32u) atomicOr(&header[(at >> 5) + 1u], value >> (32u - shift));
			at += widths[k];
		}
		__syncthreads();
	}
	for (uint32_t i = threadIdx.x; i < kSymbols; i += 256u) tables[(uint64_t) segment * kSymbols + i] = codes[i] | (lengths[i] << 16);
	if (threadIdx.x < kHeaderWords) headers[(uint64_t) segment * kHeaderWords + threadIdx.x] = header[threadIdx.x];
	if (threadIdx.x == 0u) {
		uint32_t token_bits = dynamic ? totals[0] : totals[1], block_bits = header_bits + token_bits;
		png_segment record = {header_bits, token_bits, codes[kEndOfBlock] | (lengths[kEndOfBlock] << 16), dynamic ? 1u : 0u};
		segments[segment] = record;
		// zlib header, the block, the stored block's three bits where one follows, the byte border; LEN and NLEN or Adler-32; the chunk
		chunk_sizes[segment] = (segment == 0u ? 2ull : 0ull) + (block_bits + (last ? 0u : 3u) + 7u) / 8u + 4ull + 12ull;
		if (segment == 0u) chunk_sizes[shape.segment_count] = 0ull;
	}
}

// ---- bits -------------------------------------------------------------------------------------------------------------

// the bits of a token in the code of `table` (LDS), least significant first
__device__ inline void token_code(uint32_t token, uint32_t byte, const uint32_t* table, const png_shape& shape, uint64_t& value, uint32_t& width) {
	if (token == 1u) {
		uint32_t entry = table[byte];
		value = entry & 0xFFFFu;
		width = entry >> 16;
		return;
	}
	uint32_t length = token & 511u, selector = token >> 9, index, extra_bits, extra;
	length_symbol(length, index, extra_bits, extra);
	uint32_t entry = table[257u + index];
	value = entry & 0xFFFFu;
	width = entry >> 16;
	value |= (uint64_t) extra << width;
	width += extra_bits;
	entry = table[kLiterals + distance_symbol_of(selector, shape)];
	value |= (uint64_t) (entry & 0xFFFFu) << width;
	width += entry >> 16;
	if (selector == 2u) {
		value |= (uint64_t) shape.row_extra << width;
		width += shape.row_extra_bits;
	}
}

// unit_bits[unit_count] = 0: the exclusive sum ends with the total
__global__ void __launch_bounds__(256) k_png_unit_bits(png_shape shape, const uint8_t* filtered, const uint16_t* tokens, const uint32_t* tables, uint64_t* unit_bits) {
	__shared__ uint32_t table[kSymbols];
	__shared__ uint32_t total;
	const uint32_t unit = blockIdx.x, row = unit / shape.units_per_row, first = (unit % shape.units_per_row) * kUnit;
	const uint32_t count = min(kUnit, shape.row_length - first);
	const uint64_t base = (uint64_t) row * shape.row_length + first;
	for (uint32_t i = threadIdx.x; i < kSymbols; i += 256u) table[i] = tables[(uint64_t) (row / shape.rows_per_segment) * kSymbols + i];
	if (threadIdx.x == 0u) total = 0u;
	__syncthreads();
	uint32_t bits = 0;
	for (uint32_t p = threadIdx.x; p < count; p += 256u) {
		uint32_t token = tokens[base + p];
		if (token) {
			uint64_t value;
			uint32_t width;
			token_code(token, filtered[base + p], table, shape, value, width);
			bits += width;
		}
	}
	atomicAdd(&total, bits);
	__syncthreads();
	if (threadIdx.x == 0u) {
		unit_bits[unit] = total;
		if (unit == 0u) unit_bits[shape.unit_count] = 0ull;
	}
}

// a cleared stream of `count` 32-bit words
struct bit_stream {
	uint32_t* words;
	uint64_t count;
};

// `width` <= 48 bits of `value` at bit `at` of the stream; nothing at or beyond its end is touched.  The guard is never
// taken while CAPACITY of the header holds: every token lies in front of its chunk's CRC, the last chunk in front of
// IEND, and the stream has sixteen spare bytes behind the capacity.  It is there so that a mistake in that derivation could
// not write outside the encoder's memory; such a file would fail its CRCs and the comparison with the restatement.
__device__ inline void or_bits(const bit_stream& stream, uint64_t at, uint64_t value, uint32_t width) {
	uint32_t* words = stream.words;
	uint64_t word = at >> 5;
	if (!width || word + 3u > stream.count) return;
	uint32_t shift = (uint32_t) at & 31u;
	uint32_t low = (uint32_t) (value << shift);
	uint64_t rest = shift ? value >> (32u - shift) : value >> 32;
	if (low) atomicOr(words + word, low);
	if ((uint32_t) rest) atomicOr(words + word + 1u, (uint32_t) rest);
	if (rest >> 32) atomicOr(words + word + 2u, (uint32_t) (rest >> 32));
}

// file: the words of the cleared file.  Every lane codes sixteen consecutive positions of the unit; a sum over the lanes
// places them.  The workgroup of a segment's first unit also places what surrounds the tokens.
__global__ void __launch_bounds__(256) k_png_pack(png_shape shape, const uint8_t* filtered, const uint16_t* tokens, const uint32_t* tables, const uint32_t* headers,
                                                 const png_segment* segments, const uint64_t* chunk_offsets, const uint64_t* unit_offsets, bit_stream file) {
	typedef hipcub::BlockScan<uint32_t, 256> lane_scan;
	__shared__ typename lane_scan::TempStorage scan_storage;
	__shared__ uint32_t table[kSymbols];
	const uint32_t unit = blockIdx.x, row = unit / shape.units_per_row, first = (unit % shape.units_per_row) * kUnit;
	const uint32_t count = min(kUnit, shape.row_length - first), segment = row / shape.rows_per_segment;
	const uint32_t first_unit = segment * shape.rows_per_segment * shape.units_per_row;
	const uint64_t base = (uint64_t) row * shape.row_length + first;
	for (uint32_t i = threadIdx.x; i < kSymbols; i += 256u) table[i] = tables[(uint64_t) segment * kSymbols + i];
	__syncthreads();
	const png_segment record = segments[segment];
	// the chunk's length and type, in the first chunk the zlib header
	const uint64_t data_at = VKR_PNG_HEADER_SIZE + chunk_offsets[segment] + 8u + (segment == 0u ? 2u : 0u);
	const uint64_t tokens_at = 8u * data_at + record.header_bits;
	const uint32_t begin = threadIdx.x * kPerLane, end = min(begin + kPerLane, count);
	uint64_t values[kPerLane];
	uint32_t widths[kPerLane], bits = 0;
#pragma unroll
	for (uint32_t k = 0; k != kPerLane; ++k) {
		uint32_t p = begin + k, token = p < end ? tokens[base + p] : 0u;
		values[k] = 0ull;
		widths[k] = 0u;
		if (token) token_code(token, filtered[base + p], table, shape, values[k], widths[k]);
		bits += widths[k];
	}
	uint32_t before;
	lane_scan(scan_storage).ExclusiveSum(bits, before);
	uint64_t at = tokens_at + (unit_offsets[unit] - unit_offsets[first_unit]) + before;
#pragma unroll
	for (uint32_t k = 0; k != kPerLane; ++k) {
		or_bits(file, at, values[k], widths[k]);
		at += widths[k];
	}
	if (unit != first_unit) return;
	const uint32_t* header = headers + (uint64_t) segment * kHeaderWords;
	for (uint32_t i = threadIdx.x; 8u * i < record.header_bits; i += 256u) or_bits(file, 8u * (data_at + i), (header[i >> 2] >> (8u * (i & 3u))) & 255u, 8u);
	if (threadIdx.x == 0u) {
		if (segment == 0u) or_bits(file, 8u * (data_at - 2u), 0x5E78u, 16u);
		uint32_t end_width = record.end_of_block >> 16;
		or_bits(file, tokens_at + record.token_bits - end_width, record.end_of_block & 0xFFFFu, end_width);
		if (segment + 1u != shape.segment_count) {
			// the empty stored block: 000, the byte border, LEN = 0, NLEN = FFFF
			uint64_t stored_at = data_at + (record.header_bits + record.token_bits + 3u + 7u) / 8u;
			or_bits(file, 8u * (stored_at + 2u), 0xFFFFu, 16u);
		}
	}
}

// ---- checksums and framing --------------------------------------------------------------------------------------------

constexpr uint32_t kAdlerBase = 65521u;

__device__ inline void store_big_endian(uint8_t* at, uint32_t value) {
	at[0] = (uint8_t) (value >> 24); at[1] = (uint8_t) (value >> 16); at[2] = (uint8_t) (value >> 8); at[3] = (uint8_t) value;
}

// With s1 the sum of a unit's bytes and s2 the sum of (bytes from the byte to the unit's end) * byte, the byte at position
// g of N weighs N - g in the second Adler sum: (N - the unit's end) * s1 + s2 per unit.
__global__ void __launch_bounds__(256) k_png_adler(png_shape shape, const uint32_t* unit_sums, const uint64_t* chunk_offsets, uint8_t* file) {
	__shared__ unsigned long long sums[2];
	if (threadIdx.x < 2u) sums[threadIdx.x] = 0ull;
	__syncthreads();
	uint64_t a = 0, b = 0;
	for (uint32_t unit = threadIdx.x; unit < shape.unit_count; unit += 256u) {
		uint32_t row = unit / shape.units_per_row, first = (unit % shape.units_per_row) * kUnit, count = min(kUnit, shape.row_length - first);
		uint64_t behind = shape.stream_size - ((uint64_t) row * shape.row_length + first + count);
		uint64_t s1 = unit_sums[2ull * unit], s2 = unit_sums[2ull * unit + 1u];
		a += s1;
		b = (b + (behind % kAdlerBase) * s1 + s2) % kAdlerBase;
	}
	atomicAdd(&sums[0], (unsigned long long) (a % kAdlerBase));
	atomicAdd(&sums[1], (unsigned long long) b);
	__syncthreads();
	if (threadIdx.x == 0u) {
		uint32_t low = (uint32_t) ((1ull + sums[0]) % kAdlerBase), high = (uint32_t) ((shape.stream_size % kAdlerBase + sums[1]) % kAdlerBase);
		// the last four bytes of the last chunk's data, in front of its CRC
		store_big_endian(file + VKR_PNG_HEADER_SIZE + chunk_offsets[shape.segment_count] - 8u, (high << 16) | low);
	}
}

constexpr uint32_t kCrcPolynomial = 0xEDB88320u;

// the product of two polynomials mod P, both with the coefficient of x^0 in bit 31, as CRC-32 has them
__host__ __device__ inline uint32_t multiply_mod_p(uint32_t a, uint32_t b) {
	uint32_t product = 0;
	for (uint32_t bit = 0x80000000u; bit && a; bit >>= 1) {
		if (a & bit) {
			product ^= b;
			a &= ~bit;
		}
		b = (b & 1u) ? (b >> 1) ^ kCrcPolynomial : b >> 1;
	}
	return product;
}

// x^(8 n) mod P
__host__ __device__ inline uint32_t x_to_the_bytes(uint64_t n) {
	// x^8, squared from step to step
	uint32_t power = 0x00800000u, result = 0x80000000u;
	for (; n; n >>= 1) {
		if (n & 1u) result = multiply_mod_p(power, result);
		power = multiply_mod_p(power, power);
	}
	return result;
}

__host__ __device__ inline uint32_t crc32_of(const uint8_t* data, uint64_t count) {
	uint32_t crc = 0xFFFFFFFFu;
	for (uint64_t i = 0; i != count; ++i) {
		crc ^= data[i];
		for (uint32_t k = 0; k != 8u; ++k) crc = (crc & 1u) ? (crc >> 1) ^ kCrcPolynomial : crc >> 1;
	}
	return ~crc;
}

// The CRC-32 of a string is the sum of the CRC-32 of its slices, each times x^(8 * the bytes behind the slice).
__global__ void __launch_bounds__(256) k_png_frame(png_shape shape, const uint64_t* chunk_offsets, const uint8_t* file_header, uint8_t* file, uint64_t* size_word) {
	__shared__ uint32_t combined;
	// the CRC-32 of every byte value: a step per byte instead of one per bit
	__shared__ uint32_t of_byte[256];
	{
		uint32_t entry = threadIdx.x;
		for (uint32_t k = 0; k != 8u; ++k) entry = (entry & 1u) ? (entry >> 1) ^ kCrcPolynomial : entry >> 1;
		of_byte[threadIdx.x] = entry;
	}
	const uint32_t segment = blockIdx.x;
	const uint64_t chunk_at = VKR_PNG_HEADER_SIZE + chunk_offsets[segment], data_size = chunk_offsets[segment + 1u] - chunk_offsets[segment] - 12u;
	uint8_t* chunk = file + chunk_at;
	if (threadIdx.x == 0u) {
		combined = 0u;
		store_big_endian(chunk, (uint32_t) data_size);
		chunk[4] = 'I'; chunk[5] = 'D'; chunk[6] = 'A'; chunk[7] = 'T';
	}
	if (segment == 0u && threadIdx.x < VKR_PNG_HEADER_SIZE) file[threadIdx.x] = file_header[threadIdx.x];
	if (segment + 1u == shape.segment_count) {
		const uint64_t end_at = VKR_PNG_HEADER_SIZE + chunk_offsets[shape.segment_count];
		const uint8_t end[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
		if (threadIdx.x < 12u) file[end_at + threadIdx.x] = end[threadIdx.x];
		if (threadIdx.x == 0u) *size_word = end_at + 12u;
	}
	__syncthreads();
	// type and data
	const uint64_t covered = data_size + 4u, slice = (covered + 255u) / 256u;
	const uint64_t from = min((uint64_t) threadIdx.x * slice, covered), to = min(from + slice, covered);
	uint32_t crc = 0xFFFFFFFFu;
	// (sixteen loads in flight: a lane's slice is a chain of table steps, its bytes are not)
	uint64_t i = from;
	for (; i + 16u <= to; i += 16u) {
		uint8_t bytes[16];
#pragma unroll
		for (uint32_t k = 0; k != 16u; ++k) bytes[k] = chunk[4u + i + k];
#pragma unroll
		for (uint32_t k = 0; k != 16u; ++k) crc = of_byte[(crc ^ bytes[k]) & 255u] ^ (crc >> 8);
	}
	for (; i < to; ++i) crc = of_byte[(crc ^ chunk[4u + i]) & 255u] ^ (crc >> 8);
	crc = ~crc;
	if (crc) atomicXor(&combined, multiply_mod_p(crc, x_to_the_bytes(covered - to)));
	__syncthreads();
	if (threadIdx.x == 0u) store_big_endian(chunk + 8u + data_size, combined);
}

// the file from the slot's record (output_slots.h) into memory of the caller's, of any alignment: nothing at or beyond out + capacity is written
__global__ void __launch_bounds__(256) k_png_copy_on_device(const uint8_t* record, uint8_t* out, uint64_t capacity, uint64_t* size_word) {
	uint64_t size = *(const uint64_t*) record, count = min(size, capacity);
	for (uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x; i < count; i += (uint64_t) gridDim.x * 256) out[i] = record[16u + i];
	if (blockIdx.x == 0u && threadIdx.x == 0u) *size_word = size;
}

// ---- the encoder ------------------------------------------------------------------------------------------------------

// the scratch memory of a slot besides what output_slots.h keeps
struct png_slot {
	uint8_t* filtered;
	uint16_t* tokens;
	uint32_t *histograms, *tables, *headers, *unit_sums;
	png_segment* segments;
	uint64_t *chunk_sizes, *chunk_offsets, *unit_bits, *unit_offsets;
};

struct png_state {
	// (what its slots share: the header)
	output_slots out;
	png_shape shape;
	png_slot slots[kMaxOutputSlots];
};

output_slots* slots_of(const png_encoder_t* encoder) { return encoder && encoder->state ? &((png_state*) encoder->state)->out : NULL; }

void lay_out_slot(output_carver& carve, void* png_state_pointer, uint32_t slot_index) {
	png_state* state = (png_state*) png_state_pointer;
	png_slot& slot = state->slots[slot_index];
	const size_t segments = state->shape.segment_count, units = state->shape.unit_count;
	carve.take(slot.filtered, state->shape.stream_size);
	carve.take(slot.tokens, state->shape.stream_size);
	carve.take(slot.histograms, segments * kSymbols);
	carve.take(slot.tables, segments * kSymbols);
	carve.take(slot.headers, segments * kHeaderWords);
	carve.take(slot.unit_sums, units * 2);
	carve.take(slot.segments, segments);
	carve.take(slot.chunk_sizes, segments + 1);
	carve.take(slot.chunk_offsets, segments + 1);
	carve.take(slot.unit_bits, units + 1);
	carve.take(slot.unit_offsets, units + 1);
}

bool valid_stream(uint32_t row_length, uint32_t rows) { return row_length != 0 && rows != 0 && row_length <= kMaxProbeRowLength && rows <= 65535; }

png_shape shape_of(uint32_t row_length, uint32_t rows) {
	png_shape shape;
	memset(&shape, 0, sizeof(shape));
	shape.row_length = row_length;
	shape.rows = rows;
	uint32_t fitting = VKR_PNG_SEGMENT_BYTES / row_length;
	shape.rows_per_segment = fitting < 1 ? 1 : fitting > rows ? rows : fitting;
	shape.segment_count = (rows + shape.rows_per_segment - 1) / shape.rows_per_segment;
	shape.units_per_row = (row_length + kUnit - 1) / kUnit;
	shape.unit_count = rows * shape.units_per_row;
	shape.row_candidate = row_length <= 32768;
	if (shape.row_candidate) {
		// the distance symbols of RFC 1951 3.2.5: from symbol 4 on, two symbols share each count of extra bits
		uint32_t m = row_length - 1;
		if (m < 4) shape.row_symbol = m;
		else {
			uint32_t extra_bits = 0;
			while ((m >> (extra_bits + 2)) != 0) ++extra_bits;
			shape.row_extra_bits = extra_bits;
			shape.row_symbol = 2 * extra_bits + 2 + ((m >> extra_bits) & 1);
			shape.row_extra = m & ((1u << extra_bits) - 1);
		}
	}
	shape.stream_size = (uint64_t) row_length * rows;
	return shape;
}

uint64_t capacity_of(const png_shape& shape) {
	uint64_t full = (uint64_t) shape.rows_per_segment * shape.row_length;
	uint64_t last = shape.stream_size - (uint64_t) (shape.segment_count - 1) * full;
	return VKR_PNG_HEADER_SIZE + 2 + 12 + (uint64_t) (shape.segment_count - 1) * ((9 * full + 20) / 8 + 16) + (9 * last + 20) / 8 + 16;
}

void make_header(uint8_t header[VKR_PNG_HEADER_SIZE], uint32_t width, uint32_t height) {
	const uint8_t start[16] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A, 0, 0, 0, 13, 'I', 'H', 'D', 'R'};
	memcpy(header, start, 16);
	for (uint32_t i = 0; i != 4; ++i) {
		header[16 + i] = (uint8_t) (width >> (24 - 8 * i));
		header[20 + i] = (uint8_t) (height >> (24 - 8 * i));
	}
	header[24] = 8; header[25] = 2; header[26] = header[27] = header[28] = 0;
	uint32_t crc = crc32_of(header + 12, 17);
	for (uint32_t i = 0; i != 4; ++i) header[29 + i] = (uint8_t) (crc >> (24 - 8 * i));
}

// from_stream: slot.filtered holds the stream already (the probe)
int enqueue_encode(png_encoder_t* encoder, uint32_t slot_index, const void* device_pixels, uint32_t channel_count, uint64_t row_stride_bytes, bool from_stream,
                   uint8_t* out, uint64_t capacity, uint64_t* size_word, bool copy_out, void* stream_or_null) {
	png_state* state = (png_state*) encoder->state;
	if (!state || (!from_stream && (!device_pixels || (channel_count != 3 && channel_count != 4)))) {
		printf("A PNG encode needs an encoder and device pixels of 3 or 4 bytes.\n");
		return 1;
	}
	uint64_t row_bytes = (uint64_t) encoder->width * channel_count;
	if (row_stride_bytes == 0) row_stride_bytes = row_bytes;
	if (!from_stream && row_stride_bytes < row_bytes) {
		printf("A row stride of %llu bytes is less than a row of %u pixels of %u bytes.\n", (unsigned long long) row_stride_bytes, encoder->width, channel_count);
		return 1;
	}
	hipStream_t stream;
	if (begin_output_enqueue(&state->out, slot_index, stream_or_null, &stream)) return 1;
	const png_slot& slot = state->slots[slot_index];
	const png_shape& shape = state->shape;
	uint8_t *record = state->out.slots[slot_index].record, *scan_storage = state->out.slots[slot_index].scan_storage;
	const uint64_t record_units = state->out.record_units;
	// bits are ORed into the file and counts added to the histograms
	if (hip_failed(hipMemsetAsync(record, 0, record_units * 16, stream), "clearing a PNG file")
		|| hip_failed(hipMemsetAsync(slot.histograms, 0, (size_t) shape.segment_count * kSymbols * sizeof(uint32_t), stream), "clearing the counts of a PNG encode")) return 1;
	if (!from_stream) {
		png_source source = {(const uint8_t*) device_pixels, row_stride_bytes, channel_count};
		k_png_filter<<<shape.rows, 256, 0, stream>>>(source, encoder->width, slot.filtered);
	}
	k_png_parse<<<shape.unit_count, 256, 0, stream>>>(shape, slot.filtered, slot.tokens, slot.histograms, slot.unit_sums);
	k_png_codes<<<shape.segment_count, 256, 0, stream>>>(shape, slot.histograms, slot.tables, slot.headers, slot.segments, slot.chunk_sizes);
	size_t scan_bytes = state->out.scan_bytes;
	if (hip_failed(hipcub::DeviceScan::ExclusiveSum(scan_storage, scan_bytes, slot.chunk_sizes, slot.chunk_offsets, (int) (shape.segment_count + 1), stream), "summing the sizes of the chunks")) return 1;
	k_png_unit_bits<<<shape.unit_count, 256, 0, stream>>>(shape, slot.filtered, slot.tokens, slot.tables, slot.unit_bits);
	scan_bytes = state->out.scan_bytes;
	if (hip_failed(hipcub::DeviceScan::ExclusiveSum(scan_storage, scan_bytes, slot.unit_bits, slot.unit_offsets, (int) (shape.unit_count + 1), stream), "summing the bits of the units")) return 1;
	uint8_t* file = record + 16;
	// (the words of the file and the spare sixteen bytes behind it)
	bit_stream words = {(uint32_t*) file, record_units * 4};
	k_png_pack<<<shape.unit_count, 256, 0, stream>>>(shape, slot.filtered, slot.tokens, slot.tables, slot.headers, slot.segments, slot.chunk_offsets, slot.unit_offsets, words);
	k_png_adler<<<1, 256, 0, stream>>>(shape, slot.unit_sums, slot.chunk_offsets, file);
	k_png_frame<<<shape.segment_count, 256, 0, stream>>>(shape, slot.chunk_offsets, state->out.shared, file, (uint64_t*) record);
	if (!copy_out) k_png_copy_on_device<<<256, 256, 0, stream>>>(record, out, capacity, size_word);
	return finish_output_enqueue(&state->out, slot_index, stream, copy_out ? 256 : 0);
}

int create_for_stream(png_encoder_t* encoder, const device_t* device, uint32_t row_length, uint32_t rows, uint32_t header_width, uint32_t header_height, uint32_t slot_count) {
	png_state* state = (png_state*) calloc(1, sizeof(png_state));
	if (!state) {
		printf("Out of memory creating a PNG encoder.\n");
		return 1;
	}
	const png_shape shape = shape_of(row_length, rows);
	uint8_t header[VKR_PNG_HEADER_SIZE];
	make_header(header, header_width, header_height);
	encoder->slot_count = slot_count;
	encoder->row_length = row_length;
	encoder->rows_per_segment = shape.rows_per_segment;
	encoder->segment_count = shape.segment_count;
	encoder->capacity = capacity_of(shape);
	encoder->state = state;
	state->shape = shape;
	size_t unit_scan = 0, chunk_scan = 0;
	// (sixteen spare bytes behind the record: k_png_pack ORs whole words, so up to three bytes behind the last unit of sixteen are touched, with zeros)
	int failed = hip_failed(hipcub::DeviceScan::ExclusiveSum(NULL, unit_scan, (uint64_t*) NULL, (uint64_t*) NULL, (int) (shape.unit_count + 1), (hipStream_t) device->stream), "sizing the sum of the unit bits")
		|| hip_failed(hipcub::DeviceScan::ExclusiveSum(NULL, chunk_scan, (uint64_t*) NULL, (uint64_t*) NULL, (int) (shape.segment_count + 1), (hipStream_t) device->stream), "sizing the sum of the chunk sizes")
		|| create_output_slots(&state->out, "PNG", device, slot_count, encoder->capacity, 16, unit_scan > chunk_scan ? unit_scan : chunk_scan, header, VKR_PNG_HEADER_SIZE, lay_out_slot, state);
	if (failed) destroy_png_encoder(encoder);
	return failed;
}

}  // namespace

extern "C" int get_png_header(uint8_t header[VKR_PNG_HEADER_SIZE], uint32_t width, uint32_t height) {
	if (!valid_output_extent(width, height)) return 1;
	make_header(header, width, height);
	return 0;
}

extern "C" uint64_t get_png_capacity(uint32_t width, uint32_t height) { return valid_output_extent(width, height) ? capacity_of(shape_of(3 * width + 1, height)) : 0; }

extern "C" uint64_t get_png_stream_capacity(uint32_t row_length, uint32_t rows) { return valid_stream(row_length, rows) ? capacity_of(shape_of(row_length, rows)) : 0; }

extern "C" int write_png_file(const char* path, const uint8_t* bytes, uint64_t size) { return vkr_write_file(path, bytes, size); }

extern "C" void destroy_png_encoder(png_encoder_t* encoder) {
	png_state* state = encoder ? (png_state*) encoder->state : NULL;
	if (state) {
		destroy_output_slots(&state->out);
		free(state);
	}
	if (encoder) memset(encoder, 0, sizeof(*encoder));
}

extern "C" int create_png_encoder(png_encoder_t* encoder, const device_t* device, uint32_t width, uint32_t height, uint32_t slot_count) {
	memset(encoder, 0, sizeof(*encoder));
	if (check_output_arguments("PNG", device, width, height, slot_count)) return 1;
	encoder->width = width; encoder->height = height;
	return create_for_stream(encoder, device, 3 * width + 1, height, width, height, slot_count);
}

extern "C" int begin_png_encode(png_encoder_t* encoder, uint32_t slot, const void* device_pixels, uint32_t channel_count, uint64_t row_stride_bytes, void* stream) {
	if (check_output_slot(slots_of(encoder), slot)) return 1;
	return enqueue_encode(encoder, slot, device_pixels, channel_count, row_stride_bytes, false, NULL, 0, NULL, true, stream);
}

extern "C" int end_png_encode(png_encoder_t* encoder, uint32_t slot, const uint8_t** bytes, uint64_t* size) { return end_output_encode(slots_of(encoder), slot, bytes, size); }

extern "C" int encode_png(png_encoder_t* encoder, const void* device_pixels, uint32_t channel_count, uint64_t row_stride_bytes, const uint8_t** bytes, uint64_t* size) {
	return begin_png_encode(encoder, 0, device_pixels, channel_count, row_stride_bytes, NULL) || end_png_encode(encoder, 0, bytes, size);
}

extern "C" int encode_png_on_device(png_encoder_t* encoder, const void* device_pixels, uint32_t channel_count, uint64_t row_stride_bytes,
                                    void* device_out, uint64_t capacity, uint64_t* device_size_word, void* stream) {
	if (check_output_slot(slots_of(encoder), 0)) return 1;
	if (!device_out || !device_size_word) {
		printf("encode_png_on_device() needs device memory for the file and for its size.\n");
		return 1;
	}
	return enqueue_encode(encoder, 0, device_pixels, channel_count, row_stride_bytes, false, (uint8_t*) device_out, capacity, device_size_word, false, stream);
}

extern "C" int probe_png_stream(const device_t* device, const uint8_t* host_stream, uint32_t row_length, uint32_t rows, uint8_t* out, uint64_t out_capacity, uint64_t* out_size) {
	if (!device || !host_stream || !out || !out_size || !valid_stream(row_length, rows)) {
		printf("probe_png_stream() needs a device, 1 to 65535 rows of 1 to %u bytes and memory for the file.\n", kMaxProbeRowLength);
		return 1;
	}
	png_encoder_t encoder;
	memset(&encoder, 0, sizeof(encoder));
	encoder.width = row_length; encoder.height = rows;
	if (create_for_stream(&encoder, device, row_length, rows, row_length, rows, 1)) return 1;
	png_state* state = (png_state*) encoder.state;
	const uint8_t* bytes = NULL;
	uint64_t size = 0;
	int failed = hip_failed(hipMemcpyAsync(state->slots[0].filtered, host_stream, state->shape.stream_size, hipMemcpyHostToDevice, (hipStream_t) device->stream), "uploading a filtered stream")
		|| enqueue_encode(&encoder, 0, NULL, 3, 0, true, NULL, 0, NULL, true, NULL)
		|| end_png_encode(&encoder, 0, &bytes, &size);
	if (!failed) {
		*out_size = size;
		memcpy(out, bytes, size < out_capacity ? size : out_capacity);
	}
	destroy_png_encoder(&encoder);
	return failed;
}
