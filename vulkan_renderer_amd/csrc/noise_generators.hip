// Noise tables generated on the device (include/vkr_noise_table.h generate_noise_table): the Sobol family, one thread per
// point, and void-and-cluster blue noise, one workgroup per dither array; generate_dithered_noise_table: blue-noise
// dithered sampling, one workgroup per array that anneals it in LDS, integers only.  Compiled without contraction like
// frame_statistics.hip; every table is restated in numpy bit for bit (vulkan_renderer_amd/noise_tables.py).
#include "vkr_noise_table.h"
#include "host/vkr_internal.h"
#include <hip/hip_runtime.h>

// (vkr_wang_random_number of host/noise_table.c)
__host__ __device__ static inline uint32_t wang(uint32_t seed) {
	seed = (seed ^ 61u) ^ (seed >> 16);
	seed *= 9u;
	seed ^= seed >> 4;
	seed *= 0x27d4eb2du;
	seed ^= seed >> 15;
	return seed;
}

// ---- Sobol family ------------------------------------------------------------------------------------------------

constexpr uint32_t kSobolBlock = 256;

struct sobol_args {
	// direction numbers v[d][k] and the seeds of the four dimensions
	uint32_t v[4][32];
	uint32_t seed[4];
	// W = H = 2^m
	uint32_t m;
	noise_type_t type;
	uint64_t point_count;
	uint32_t* table;
};

// Output bit b, counted from the top, is flipped by the top bit of wang(wang(node) ^ seed), node = (1 << b) | the b bits
// above: only the `bits` bits a texel uses are computed, the others do not enter them
__device__ static inline uint32_t owen_scramble(uint32_t x, uint32_t seed, uint32_t bits) {
	uint32_t out = 0;
	for (uint32_t b = 0; b != bits; ++b) {
		uint32_t prefix = b ? x >> (32 - b) : 0u;
		uint32_t flip = wang(wang(prefix | (1u << b)) ^ seed) >> 31;
		out |= (((x >> (31 - b)) & 1u) ^ flip) << (31 - b);
	}
	return out;
}

__device__ static inline uint32_t laine_karras(uint32_t x, uint32_t seed) {
	x += seed;
	x ^= x * 0x6c50b47cu;
	x ^= x * 0xb82f1e52u;
	x ^= x * 0xc7afe638u;
	x ^= x * 0x8d22f6e6u;
	return x;
}

// One lane per point: every block of W * H consecutive points writes every texel of its layer and channel pair once
__global__ void __launch_bounds__(kSobolBlock) k_sobol_points(sobol_args a) {
	uint64_t g = (uint64_t) blockIdx.x * kSobolBlock + threadIdx.x;
	if (g >= a.point_count) return;
	uint32_t i = (uint32_t) g;
	uint32_t c[4] = {0u, 0u, 0u, 0u};
#pragma unroll
	for (uint32_t k = 0; k != 32; ++k)
		if ((i >> k) & 1u) {
#pragma unroll
			for (uint32_t d = 0; d != 4; ++d) c[d] ^= a.v[d][k];
		}
	if (a.type == noise_type_owen) {
#pragma unroll
		for (uint32_t d = 0; d != 4; ++d) c[d] = owen_scramble(c[d], a.seed[d], d < 2 ? a.m : 16u);
	}
	else if (a.type == noise_type_burley_owen) {
#pragma unroll
		for (uint32_t d = 0; d != 4; ++d) c[d] = __brev(laine_karras(__brev(c[d]), a.seed[d]));
	}
	uint32_t m = a.m;
	uint64_t block = g >> (2 * m);
	uint32_t x = c[0] >> (32 - m), y = c[1] >> (32 - m);
	uint64_t texel = ((block >> 1) << (2 * m)) + ((uint64_t) y << m) + x;
	a.table[texel * 2 + (block & 1)] = (c[2] >> 16) | (c[3] & 0xFFFF0000u);
}

static void fill_direction_numbers(uint32_t v[4][32]) {
	// (s, a, m) of Joe and Kuo for dimensions 1 ... 3; dimension 0 is van der Corput
	static const uint32_t degree[3] = {1, 2, 3}, polynomial[3] = {0, 1, 1}, initial[3][3] = {{1, 0, 0}, {1, 3, 0}, {1, 3, 1}};
	for (uint32_t k = 0; k != 32; ++k) v[0][k] = 1u << (31 - k);
	for (uint32_t d = 1; d != 4; ++d) {
		uint32_t s = degree[d - 1], a = polynomial[d - 1];
		for (uint32_t k = 0; k != 32; ++k) {
			if (k < s) { v[d][k] = initial[d - 1][k] << (31 - k); continue; }
			uint32_t value = v[d][k - s] ^ (v[d][k - s] >> s);
			for (uint32_t j = 1; j < s; ++j)
				if ((a >> (s - 1 - j)) & 1u) value ^= v[d][k - j];
			v[d][k] = value;
		}
	}
}

// ---- blue noise ----------------------------------------------------------------------------------------------------

constexpr uint32_t kMaxWaves = 16;

struct blue_args {
	uint32_t width, height, log2_width, log2_count;
	uint32_t seed;
	// K of the header, height * width floats
	const float* kernel;
	// width * height floats per array: the energies of the prototype pattern while its ones are ranked
	float* scratch;
	uint16_t* table;
};

// The workgroup's view of one array.  Pixel p belongs to thread p % T as its pixel number p / T: a thread's energies are
// E[t], E[t + T], ... (consecutive lanes, consecutive banks), its part of the pattern the bits of `mask`.
template <uint32_t T> struct blue_state {
	float* E;
	const float* K;
	float* reduced_value;
	uint32_t* reduced_index;
	uint32_t width_mask, height_mask, log2_width;
	uint32_t t, pixels;
	uint32_t mask, parity;

	__device__ inline uint32_t kernel_index(uint32_t p, uint32_t ux, uint32_t uy) const {
		return ((((p >> log2_width) - uy) & height_mask) << log2_width) + (((p & width_mask) - ux) & width_mask);
	}

	__device__ inline void set(uint32_t p, bool one) {
		if ((p & (T - 1)) != t) return;
		uint32_t bit = 1u << (p / T);
		mask = one ? (mask | bit) : (mask & ~bit);
	}

	// (value, index) pairs reduce lexicographically: ties of the extreme go to the lowest pixel
	template <bool MAXIMUM> __device__ static inline bool better(float v, uint32_t i, float best, uint32_t best_i) {
		return (MAXIMUM ? v > best : v < best) || (v == best && i < best_i);
	}

	// One pass: adds sign * K centred on pixel u to every energy (sign 0: no update) and finds the tightest cluster
	// (CLUSTER: the maximum among the ones) or the largest void (the minimum among the zeros) of what results.
	// One barrier; every thread returns the same pixel.
	template <bool CLUSTER> __device__ inline uint32_t step(uint32_t u, int sign) {
		float best = CLUSTER ? -INFINITY : INFINITY;
		uint32_t best_i = 0xFFFFFFFFu;
		uint32_t ux = u & width_mask, uy = u >> log2_width;
		// (four pixels at a time: their LDS reads are independent and overlap)
#pragma unroll 4
		for (uint32_t j = 0; j != pixels; ++j) {
			uint32_t p = t + j * T;
			float e = E[p];
			if (sign) {
				float k = K[kernel_index(p, ux, uy)];
				e = sign > 0 ? e + k : e - k;
				E[p] = e;
			}
			bool one = (mask >> j) & 1u;
			// (a thread's pixels ascend: the strict comparison keeps the lowest)
			if (one == CLUSTER && (CLUSTER ? e > best : e < best)) { best = e; best_i = p; }
		}
		for (uint32_t offset = 32; offset != 0; offset >>= 1) {
			float v = __shfl_xor(best, offset);
			uint32_t i = __shfl_xor(best_i, offset);
			if (better<CLUSTER>(v, i, best, best_i)) { best = v; best_i = i; }
		}
		// two sets of slots: a wave that is a step ahead writes the other one
		uint32_t slot = parity * kMaxWaves;
		parity ^= 1u;
		if ((threadIdx.x & 63u) == 0) {
			reduced_value[slot + (threadIdx.x >> 6)] = best;
			reduced_index[slot + (threadIdx.x >> 6)] = best_i;
		}
		__syncthreads();
		best = reduced_value[slot];
		best_i = reduced_index[slot];
		for (uint32_t w = 1; w != T / 64; ++w) {
			float v = reduced_value[slot + w];
			uint32_t i = reduced_index[slot + w];
			if (better<CLUSTER>(v, i, best, best_i)) { best = v; best_i = i; }
		}
		return best_i;
	}
};

template <uint32_t T> __global__ void __launch_bounds__(T) k_blue_arrays(blue_args a) {
	extern __shared__ __align__(16) unsigned char lds[];
	const uint32_t N = 1u << a.log2_count, n1 = N / 10, word_count = (N + 63) / 64;
	const uint32_t array = blockIdx.x, t = threadIdx.x;
	blue_state<T> s;
	s.E = (float*) lds;
	float* K = s.E + N;
	s.K = K;
	unsigned long long* words = (unsigned long long*) (K + N);
	s.reduced_value = (float*) (words + word_count);
	s.reduced_index = (uint32_t*) (s.reduced_value + 2 * kMaxWaves);
	s.width_mask = a.width - 1; s.height_mask = a.height - 1; s.log2_width = a.log2_width;
	s.t = t;
	// (threads beyond the array own nothing and only take part in the barriers)
	s.pixels = t < N ? (N >= T ? N / T : 1u) : 0u;
	s.mask = 0; s.parity = 0;
	uint32_t* keys = (uint32_t*) s.E;
	const uint32_t key_base = wang(wang(a.seed) + array);
	for (uint32_t j = 0; j != s.pixels; ++j) {
		uint32_t p = t + j * T;
		K[p] = a.kernel[p];
		keys[p] = wang(key_base + p);
	}
	__syncthreads();
	// 1. the ones are the n1 pixels with the smallest (key, pixel)
	for (uint32_t j = 0; j != s.pixels; ++j) {
		uint32_t p = t + j * T, key = keys[p], smaller = 0;
		for (uint32_t q = 0; q != N; ++q) {
			uint32_t other = keys[q];
			smaller += (other < key || (other == key && q < p)) ? 1u : 0u;
		}
		if (smaller < n1) s.mask |= 1u << j;
	}
	__syncthreads();
	float* saved = a.scratch + (size_t) array * N;
	uint16_t* out = a.table + (((size_t) (array >> 2) * N) << 2) + (array & 3u);
	uint32_t c = 0, v = 0;
	for (int pass = 0; pass != 2; ++pass) {
		// the energy of the ones, added in ascending pixel order (pass 1: of the inverted pattern, step 5)
		for (uint32_t j = 0; j * T < N; ++j) {
			unsigned long long word = __ballot(j < s.pixels && ((s.mask >> j) & 1u));
			uint32_t first = j * T + (t & ~63u);
			if ((t & 63u) == 0 && first < N) words[first / 64] = word;
		}
		__syncthreads();
		for (uint32_t j = 0; j != s.pixels; ++j) {
			uint32_t p = t + j * T;
			float e = 0.0f;
			for (uint32_t w = 0; w != word_count; ++w)
				for (unsigned long long bits = words[w]; bits; bits &= bits - 1) {
					uint32_t q = w * 64 + (uint32_t) __builtin_ctzll(bits);
					e += K[s.kernel_index(p, q & s.width_mask, q >> s.log2_width)];
				}
			s.E[p] = e;
		}
		c = s.template step<true>(0, 0);
		if (pass == 1) {
			// 5. the ones of the inverted pattern, tightest cluster first
			for (uint32_t r = N / 2; r != N; ++r) {
				if ((c & (T - 1)) == t) out[(size_t) c << 2] = (uint16_t) ((r * 65536u + 32768u) >> a.log2_count);
				s.set(c, false);
				if (r + 1 != N) c = s.template step<true>(c, -1);
			}
			break;
		}
		// 2. relax: the tightest cluster moves into the largest void until it is its own largest void (at most N times)
		for (uint32_t rounds = 1; ; ++rounds) {
			s.set(c, false);
			v = s.template step<false>(c, -1);
			if (v == c || rounds == N) {
				s.set(c, true);
				c = s.template step<true>(c, 1);
				break;
			}
			s.set(v, true);
			c = s.template step<true>(v, 1);
		}
		// 3. on a copy: the ones of the prototype, tightest cluster first
		uint32_t prototype = s.mask;
		for (uint32_t j = 0; j != s.pixels; ++j) saved[t + j * T] = s.E[t + j * T];
		for (uint32_t r = n1; r-- != 0; ) {
			if ((c & (T - 1)) == t) out[(size_t) c << 2] = (uint16_t) ((r * 65536u + 32768u) >> a.log2_count);
			s.set(c, false);
			if (r) c = s.template step<true>(c, -1);
		}
		// 4. the prototype again: the largest void is filled until half of the pixels are ones
		s.mask = prototype;
		// (each thread reads back what it wrote itself)
		for (uint32_t j = 0; j != s.pixels; ++j) s.E[t + j * T] = saved[t + j * T];
		v = s.template step<false>(0, 0);
		for (uint32_t r = n1; r != N / 2; ++r) {
			if ((v & (T - 1)) == t) out[(size_t) v << 2] = (uint16_t) ((r * 65536u + 32768u) >> a.log2_count);
			s.set(v, true);
			if (r + 1 != N / 2) v = s.template step<false>(v, 1);
		}
		s.mask = ~s.mask & ((1u << s.pixels) - 1u);
		// (the words are read by everyone until the barrier of the last step above)
		__syncthreads();
	}
}

// ---- blue-noise dithered sampling ----------------------------------------------------------------------------------

constexpr uint32_t kDitheredRadius = 6, kDitheredSide = 2 * kDitheredRadius + 1, kDitheredWindow = kDitheredSide * kDitheredSide;
constexpr uint32_t kDitheredValueWeights = 1449;

struct dithered_args {
	uint32_t log2_width, log2_height;
	uint32_t seed;
	uint32_t first_round, round_count;
	// v[1][b] of the Sobol sequence for the bits b of a point index
	uint32_t direction[16];
	// Kq, then Gq
	const uint32_t* weights;
	// the table as packed values x | y << 16: word 2 * (layer * N + pixel) + pair
	uint32_t* table;
};

__device__ static inline uint32_t* dithered_array_values(const dithered_args& a, uint32_t array) {
	return a.table + ((((size_t) (array >> 1)) << (a.log2_width + a.log2_height)) << 1) + (array & 1u);
}

// The initial assignment, one lane per pixel: its rank j among the keys, then point j of the value set
__global__ void __launch_bounds__(256) k_dithered_initial(dithered_args a) {
	const uint32_t N = 1u << (a.log2_width + a.log2_height);
	const uint32_t array = blockIdx.x, pixel = blockIdx.y * 256 + threadIdx.x;
	const uint32_t s = wang(wang(a.seed) + array);
	uint32_t key = wang(s + pixel), j = 0;
	for (uint32_t q = 0; q != N; ++q) {
		uint32_t other = wang(s + q);
		j += (other < key || (other == key && q < pixel)) ? 1u : 0u;
	}
	// (dimension 0 is van der Corput: the XOR of 2^(31 - b) over the set bits b)
	uint32_t c0 = __brev(j), c1 = 0;
#pragma unroll
	for (uint32_t b = 0; b != 16; ++b)
		if ((j >> b) & 1u) c1 ^= a.direction[b];
	uint32_t x = owen_scramble(c0, wang(s + 0x9E3779B9u), 16) >> 16;
	uint32_t y = owen_scramble(c1, wang(s + 0x9E3779B9u * 2u), 16) >> 16;
	dithered_array_values(a, array)[(size_t) pixel * 2] = x | (y << 16);
}

// Toroidal distance of two 16-bit coordinates held in the upper halves of a and b: min(|d|, 65536 - |d|) is the magnitude
// of the difference as a signed 16-bit number
__device__ static inline uint32_t dithered_axis_distance(uint32_t a_upper, uint32_t b_upper) {
	int d = (int) (a_upper - b_upper) >> 16;
	return (uint32_t) (d < 0 ? -d : d);
}

// (__umul24 returns an int)
__device__ static inline uint32_t dithered_mul24(uint32_t a, uint32_t b) { return (uint32_t) __umul24(a, b); }

// Gq's index of a value and a neighbour, both as (x << 16, y << 16): r >> 5 with r the largest integer whose square is at
// most ax^2 + ay^2 <= 2^31.  The square root instruction is within 0.01 of the root, so its floor is at most one off.
// (Every factor is below 2^24: the 24-bit multiplier runs at the full rate, the 32-bit one does not.)
__device__ static inline uint32_t dithered_value_index(uint32_t ax_upper, uint32_t ay_upper, uint32_t bx_upper, uint32_t by_upper) {
	uint32_t ax = dithered_axis_distance(ax_upper, bx_upper), ay = dithered_axis_distance(ay_upper, by_upper);
	uint32_t squared = dithered_mul24(ax, ax) + dithered_mul24(ay, ay);
	uint32_t r = (uint32_t) __builtin_amdgcn_sqrtf((float) squared), rr = dithered_mul24(r, r);
	// (at most one of the two holds; (r + 1)^2 = rr + 2 r + 1)
	return (r - (rr > squared ? 1u : 0u) + (rr + 2u * r + 1u <= squared ? 1u : 0u)) >> 5;
}

// One workgroup per array, G lanes per swap: blockDim.x = G * T / 2 with T the tile count, G a divisor of 64.  The values
// of the array stay in LDS for round_count rounds.  The 169 entries of a window are dealt to the lanes of a swap once,
// before the first round; a lane sums its part of delta, first around p, then around q, the group adds up by shuffles
// and lane 0 exchanges the values.  One barrier per round: no window of a round holds a pixel that the round may change.
template <uint32_t G> __global__ void __launch_bounds__(1024) k_dithered_rounds(dithered_args a) {
	extern __shared__ __align__(16) unsigned char lds[];
	constexpr uint32_t kSteps = (kDitheredWindow + G - 1) / G;
	const uint32_t log2_width = a.log2_width, N = 1u << (log2_width + a.log2_height);
	const uint32_t width_mask = (1u << log2_width) - 1u, height_mask = (1u << a.log2_height) - 1u;
	const uint32_t tiles = N >> 8, tiles_x_mask = (width_mask >> 4), log2_tiles_x = log2_width - 4;
	uint32_t* V = (uint32_t*) lds;
	uint32_t* Gq = V + N;
	const uint32_t array = blockIdx.x, lane = threadIdx.x % G, swap = threadIdx.x / G;
	uint32_t* values = dithered_array_values(a, array);
	for (uint32_t i = threadIdx.x; i < N; i += blockDim.x) V[i] = values[(size_t) i * 2];
	for (uint32_t i = threadIdx.x; i < kDitheredValueWeights; i += blockDim.x) Gq[i] = a.weights[kDitheredWindow + i];
	// entry w = lane + G * j of either window: the offsets to add to the centre modulo W and H, and Kq; entries past the
	// end have weight 0
	uint32_t offset_x[kSteps], offset_y[kSteps], weight[kSteps];
#pragma unroll
	for (uint32_t j = 0; j != kSteps; ++j) {
		uint32_t w = lane + G * j;
		bool valid = w < kDitheredWindow;
		if (!valid) w = 0;
		offset_x[j] = (w % kDitheredSide - kDitheredRadius) & width_mask;
		offset_y[j] = (w / kDitheredSide - kDitheredRadius) & height_mask;
		weight[j] = valid ? a.weights[w] : 0u;
	}
	const uint32_t s = wang(wang(a.seed) + array), grid_base = wang(s ^ 0x9E3779B9u);
	__syncthreads();
	for (uint32_t k = a.first_round; k != a.first_round + a.round_count; ++k) {
		uint32_t g = wang(grid_base + k), tile_base = wang(s + k);
		uint32_t mask = 1u + ((((g >> 8) & 0xFFFFu) * (tiles - 1u)) >> 16);
		// the pairs (t, t ^ mask) with t < t ^ mask: the highest bit of the mask is clear in t
		uint32_t high = 31u - (uint32_t) __clz((int) mask);
		uint32_t tile[2], x[2], y[2], pixel[2], value[2];
		tile[0] = ((swap >> high) << (high + 1u)) | (swap & ((1u << high) - 1u));
		tile[1] = tile[0] ^ mask;
#pragma unroll
		for (uint32_t i = 0; i != 2; ++i) {
			uint32_t h = wang(tile_base + tile[i]);
			x[i] = (16u * (tile[i] & tiles_x_mask) + (g & 15u) + (((h & 0xFFFFu) * 10u) >> 16)) & width_mask;
			y[i] = (16u * (tile[i] >> log2_tiles_x) + ((g >> 4) & 15u) + (((h >> 16) * 10u) >> 16)) & height_mask;
			pixel[i] = (y[i] << log2_width) | x[i];
			value[i] = V[pixel[i]];
		}
		const uint32_t value_x[2] = {value[0] << 16, value[1] << 16}, value_y[2] = {value[0] & 0xFFFF0000u, value[1] & 0xFFFF0000u};
		long long delta = 0;
#pragma unroll
		for (uint32_t i = 0; i != 2; ++i) {
#pragma unroll
			for (uint32_t j = 0; j != kSteps; ++j) {
				uint32_t nx = (x[i] + offset_x[j]) & width_mask, ny = (y[i] + offset_y[j]) & height_mask;
				uint32_t neighbour = V[(ny << log2_width) | nx];
				uint32_t neighbour_x = neighbour << 16, neighbour_y = neighbour & 0xFFFF0000u;
				// the pixel's own value leaves, the other one comes (32-bit products, 64-bit sum)
				uint32_t comes = Gq[dithered_value_index(value_x[1 - i], value_y[1 - i], neighbour_x, neighbour_y)];
				uint32_t leaves = Gq[dithered_value_index(value_x[i], value_y[i], neighbour_x, neighbour_y)];
				delta += (long long) dithered_mul24(weight[j], comes) - (long long) dithered_mul24(weight[j], leaves);
			}
		}
#pragma unroll
		for (uint32_t offset = G / 2; offset != 0; offset >>= 1) delta += __shfl_xor(delta, (int) offset);
		if (lane == 0 && delta < 0) {
			V[pixel[0]] = value[1];
			V[pixel[1]] = value[0];
		}
		__syncthreads();
	}
	for (uint32_t i = threadIdx.x; i < N; i += blockDim.x) values[(size_t) i * 2] = V[i];
}

static uint32_t log2_of(uint32_t x) {
	uint32_t l = 0;
	while ((1u << l) < x) ++l;
	return l;
}

static int is_power_of_two(uint32_t x) { return x && !(x & (x - 1)); }

static int generate_sobol(void* table, hipStream_t stream, VkExtent3D resolution, noise_type_t type, uint32_t generator_seed) {
	sobol_args args;
	fill_direction_numbers(args.v);
	for (uint32_t d = 0; d != 4; ++d) args.seed[d] = wang(generator_seed + 0x9E3779B9u * (d + 1));
	args.m = log2_of(resolution.width);
	args.type = type;
	args.point_count = 2ull * resolution.depth * resolution.width * resolution.height;
	args.table = (uint32_t*) table;
	k_sobol_points<<<(uint32_t) ((args.point_count + kSobolBlock - 1) / kSobolBlock), kSobolBlock, 0, stream>>>(args);
	return hip_failed(hipGetLastError(), "generating Sobol points");
}

static int generate_blue(void* table, hipStream_t stream, VkExtent3D resolution, uint32_t generator_seed) {
	uint32_t W = resolution.width, H = resolution.height, N = W * H, array_count = 4 * resolution.depth;
	// K[dy][dx] = (float) exp(-(dx^2 + dy^2) / (2 * 1.5^2)) over toroidal distances, in double on the host
	float* kernel_host = (float*) malloc(sizeof(float) * N);
	float* kernel = NULL;
	float* scratch = NULL;
	if (!kernel_host || hipMalloc(&kernel, sizeof(float) * N) != hipSuccess || hipMalloc(&scratch, sizeof(float) * (size_t) N * array_count) != hipSuccess) {
		printf("Failed to allocate the temporary buffers of %u blue noise arrays of %ux%u.\n", array_count, W, H);
		free(kernel_host);
		if (kernel) (void) hipFree(kernel);
		return 1;
	}
	for (uint32_t y = 0; y != H; ++y)
		for (uint32_t x = 0; x != W; ++x) {
			double dx = (double) (x < W - x ? x : W - x), dy = (double) (y < H - y ? y : H - y);
			kernel_host[y * W + x] = (float) exp(-(dx * dx + dy * dy) / (2.0 * 1.5 * 1.5));
		}
	blue_args args;
	args.width = W; args.height = H; args.log2_width = log2_of(W); args.log2_count = log2_of(N);
	args.seed = generator_seed;
	args.kernel = kernel; args.scratch = scratch; args.table = (uint16_t*) table;
	// energies, K, the pattern as 64-bit words, two sets of reduction slots
	size_t lds_bytes = sizeof(float) * 2 * (size_t) N + 8 * (size_t) ((N + 63) / 64) + 2 * kMaxWaves * 8;
	int failed = hip_failed(hipMemcpyAsync(kernel, kernel_host, sizeof(float) * N, hipMemcpyHostToDevice, stream), "uploading the energy kernel");
	// 16 pixels per thread at most (their part of the pattern is the bits of one register)
	if (!failed && N <= 4096) {
		k_blue_arrays<256><<<array_count, 256, lds_bytes, stream>>>(args);
		failed = hip_failed(hipGetLastError(), "generating blue noise");
	}
	else if (!failed) {
		// (64 KiB of energies and as much of K: beyond the default limit of a workgroup)
		failed = hip_failed(hipFuncSetAttribute((const void*) k_blue_arrays<1024>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds_bytes), "raising the LDS limit of the blue noise kernel");
		if (!failed) {
			k_blue_arrays<1024><<<array_count, 1024, lds_bytes, stream>>>(args);
			failed = hip_failed(hipGetLastError(), "generating blue noise");
		}
	}
	// (the kernel and the upload read the temporaries)
	failed = hip_failed(hipStreamSynchronize(stream), "generating blue noise") || failed;
	(void) hipFree(kernel);
	(void) hipFree(scratch);
	free(kernel_host);
	return failed;
}

extern "C" int generate_noise_table(noise_table_t* noise, const device_t* device, VkExtent3D resolution, noise_type_t noise_type, uint32_t generator_seed) {
	memset(noise, 0, sizeof(*noise));
	uint32_t W = resolution.width, H = resolution.height, D = resolution.depth;
	if (!device) {
		printf("generate_noise_table() needs a device: the generators are HIP kernels.\n");
		return 1;
	}
	int sobol_family = noise_type == noise_type_sobol || noise_type == noise_type_owen || noise_type == noise_type_burley_owen;
	if (!sobol_family && noise_type != noise_type_blue) {
		printf("generate_noise_table() generates the types blue, sobol, owen and burley_owen; type %d is loaded by load_noise_table().\n", (int) noise_type);
		return 1;
	}
	if (sobol_family && !(W == H && is_power_of_two(W) && W >= 4 && W <= 4096 && is_power_of_two(D) && 2ull * D * W * H <= (1ull << 32))) {
		printf("A Sobol table needs W = H = 2^m with 2 <= m <= 12, D a power of two and 2 D W H <= 2^32, not %ux%ux%u.\n", W, H, D);
		return 1;
	}
	if (!sobol_family && !(is_power_of_two(W) && is_power_of_two(H) && W >= 4 && W <= 128 && H >= 4 && H <= 128 && is_power_of_two(D) && D <= (1u << 24))) {
		printf("A blue noise table needs W and H powers of two in 4 ... 128 and D a power of two, not %ux%ux%u.\n", W, H, D);
		return 1;
	}
	size_t bytes = sizeof(uint16_t) * 4 * (size_t) W * H * D;
	hipStream_t stream = (hipStream_t) device->stream;
	noise->host_data = (uint16_t*) malloc(bytes);
	int failed = !noise->host_data || vkr_device_alloc(&noise->device_data, device, bytes, "the noise table");
	if (!noise->host_data) printf("Out of memory for a noise table of %llu bytes.\n", (unsigned long long) bytes);
	failed = failed || (sobol_family ? generate_sobol(noise->device_data, stream, resolution, noise_type, generator_seed) : generate_blue(noise->device_data, stream, resolution, generator_seed))
		|| vkr_copy_to_host(noise->host_data, noise->device_data, bytes, device);
	if (failed) {
		destroy_noise_table(noise, device);
		return 1;
	}
	noise->resolution = resolution;
	noise->random_seed = 3124705;
	return 0;
}

extern "C" void get_dithered_noise_weights(uint32_t spatial[169], uint32_t value[1449]) {
	for (uint32_t w = 0; w != kDitheredWindow; ++w) {
		double dx = (double) (w % kDitheredSide) - (double) kDitheredRadius, dy = (double) (w / kDitheredSide) - (double) kDitheredRadius;
		spatial[w] = (uint32_t) rint(65536.0 * exp(-(dx * dx + dy * dy) / (2.1 * 2.1)));
	}
	spatial[kDitheredWindow / 2] = 0;
	for (uint32_t i = 0; i != kDitheredValueWeights; ++i)
		value[i] = (uint32_t) rint(65536.0 * exp(-(((double) i + 0.5) / 2048.0) / (1.0 * 1.0)));
}

extern "C" uint32_t get_default_dithered_round_count(VkExtent3D resolution) {
	// A round offers one pixel per 16x16 tile whatever the resolution, so the rounds a pixel needs do not grow with
	// the table; measured at 128x128, where 2^20 rounds gain 0.9 % over these
	(void) resolution;
	return 1u << 19;
}

template <uint32_t G> static int launch_dithered_rounds(const dithered_args& args, uint32_t array_count, uint32_t threads, size_t lds_bytes, hipStream_t stream) {
	// (64 KiB of values and the value weights at 128x128: beyond the default limit of a workgroup)
	if (hip_failed(hipFuncSetAttribute((const void*) k_dithered_rounds<G>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds_bytes), "raising the LDS limit of the dithered sampling kernel"))
		return 1;
	k_dithered_rounds<G><<<array_count, threads, lds_bytes, stream>>>(args);
	return hip_failed(hipGetLastError(), "annealing the dithered sampling table");
}

extern "C" int generate_dithered_noise_table(noise_table_t* noise, const device_t* device, VkExtent3D resolution, uint32_t generator_seed, uint32_t round_count) {
	memset(noise, 0, sizeof(*noise));
	uint32_t W = resolution.width, H = resolution.height, D = resolution.depth;
	if (!device) {
		printf("generate_dithered_noise_table() needs a device: the generator is a HIP kernel.\n");
		return 1;
	}
	if (!(is_power_of_two(W) && is_power_of_two(H) && W >= 16 && W <= 256 && H >= 16 && H <= 256 && W * H >= 512 && W * H <= 32768 && is_power_of_two(D) && D <= (1u << 24))) {
		printf("A dithered sampling table needs W and H powers of two in 16 ... 256 with 512 <= W H <= 32768 and D a power of two, not %ux%ux%u.\n", W, H, D);
		return 1;
	}
	if (round_count > (1u << 22)) {
		printf("A dithered sampling table takes at most %u rounds, not %u.\n", 1u << 22, round_count);
		return 1;
	}
	uint32_t N = W * H, array_count = 2 * D, swap_count = N / 512;
	size_t bytes = sizeof(uint16_t) * 4 * (size_t) N * D;
	hipStream_t stream = (hipStream_t) device->stream;
	uint32_t weights_host[kDitheredWindow + kDitheredValueWeights];
	get_dithered_noise_weights(weights_host, weights_host + kDitheredWindow);
	uint32_t v[4][32];
	fill_direction_numbers(v);
	dithered_args args;
	args.log2_width = log2_of(W); args.log2_height = log2_of(H);
	args.seed = generator_seed;
	args.first_round = 0; args.round_count = 0;
	for (uint32_t b = 0; b != 16; ++b) args.direction[b] = v[1][b];
	uint32_t* weights = NULL;
	noise->host_data = (uint16_t*) malloc(bytes);
	if (!noise->host_data) printf("Out of memory for a noise table of %llu bytes.\n", (unsigned long long) bytes);
	int failed = !noise->host_data || vkr_device_alloc(&noise->device_data, device, bytes, "the noise table")
		|| hip_failed(hipMalloc(&weights, sizeof(weights_host)), "allocating the weights of the dithered sampling table")
		|| hip_failed(hipMemcpyAsync(weights, weights_host, sizeof(weights_host), hipMemcpyHostToDevice, stream), "uploading the weights of the dithered sampling table");
	args.weights = weights; args.table = (uint32_t*) noise->device_data;
	if (!failed) {
		k_dithered_initial<<<dim3(array_count, N / 256), 256, 0, stream>>>(args);
		failed = hip_failed(hipGetLastError(), "assigning the values of the dithered sampling table");
	}
	// as many lanes per swap as a workgroup of 1024 has for it, at most a wave
	size_t lds_bytes = sizeof(uint32_t) * ((size_t) N + kDitheredValueWeights);
	for (uint32_t first = 0; !failed && first < round_count; first += VKR_DITHERED_ROUNDS_PER_LAUNCH) {
		args.first_round = first;
		args.round_count = round_count - first < VKR_DITHERED_ROUNDS_PER_LAUNCH ? round_count - first : VKR_DITHERED_ROUNDS_PER_LAUNCH;
		if (swap_count <= 16) failed = launch_dithered_rounds<64>(args, array_count, 64 * swap_count, lds_bytes, stream);
		else if (swap_count == 32) failed = launch_dithered_rounds<32>(args, array_count, 1024, lds_bytes, stream);
		else failed = launch_dithered_rounds<16>(args, array_count, 1024, lds_bytes, stream);
	}
	// (the upload reads weights_host, the kernels the weights)
	failed = hip_failed(hipStreamSynchronize(stream), "generating the dithered sampling table") || failed;
	if (weights) (void) hipFree(weights);
	failed = failed || vkr_copy_to_host(noise->host_data, noise->device_data, bytes, device);
	if (failed) {
		destroy_noise_table(noise, device);
		return 1;
	}
	noise->resolution = resolution;
	noise->random_seed = 3124705;
	return 0;
}
