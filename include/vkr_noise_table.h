/* Tabulated noise: reference src/noise_table.h:21-89. */
#ifndef VKR_NOISE_TABLE_H
#define VKR_NOISE_TABLE_H
#include "vkr_device.h"

/*! Same values as reference noise_table.h:21-55 */
typedef enum noise_type_e {
	noise_type_white = 0,
	noise_type_blue,
	noise_type_ahmed,
	noise_type_count,
	noise_type_sobol,
	noise_type_owen,
	noise_type_burley_owen,
	noise_type_blue_noise_dithered,
	noise_type_full_count,
} noise_type_t;

typedef struct noise_table_s {
	/*! RGBA16_UNORM, layer-major: depth * height * width * 4 uint16_t */
	VkExtent3D resolution;
	uint16_t* host_data;
	void* device_data;
	/*! Seed for the per-frame randomisation (reference noise_table.h:66) */
	uint32_t random_seed;
} noise_table_t;

/*! reference noise_table.h:71 / noise_table.c:23-43 */
VKR_API VkExtent3D get_default_noise_resolution(noise_type_t noise_type);
/*! reference noise_table.h:81 / noise_table.c:46-153.  White noise is generated;
	every other type is read from data/noise/<type>_..._<W>x<H>_<D>.blob relative to
	the working directory, exactly like the reference. */
VKR_API int load_noise_table(noise_table_t* noise, const device_t* device, VkExtent3D resolution, noise_type_t noise_type);
/*! reference noise_table.h:84 */
VKR_API void destroy_noise_table(noise_table_t* noise, const device_t* device);
/*! reference noise_table.h:89 / noise_table.c:161-168 */
VKR_API void set_noise_constants(uint32_t resolution_mask[2], uint32_t* texture_index_mask, uint32_t random_numbers[4], noise_table_t* noise, VkBool32 animate_noise);

/* ---- tables generated on the device (no reference counterpart: the reference reads these tables from downloaded blobs) ----

   generate_noise_table() fills device_data by HIP kernels (csrc/noise_generators.hip, on device->stream), host_data by one
   read-back, sets resolution and random_seed = 3124705 like load_noise_table() and returns 0.  It returns 1 after printing
   one line, with the struct zeroed, for: device == NULL (there is no host build of the generators), noise_type_white
   (load_noise_table() generates it), noise_type_ahmed (a blob type), noise_type_blue_noise_dithered (its annealing needs a
   round count: generate_dithered_noise_table() below), and resolutions outside the ranges below.  The rules that follow, the order of operations included, are the interface: the numpy
   restatement vulkan_renderer_amd/noise_tables.py gives the same bytes.  wang() is vkr_wang_random_number (reference
   math_utilities.h:50-57); all integers are uint32_t.

   noise_type_sobol, noise_type_owen, noise_type_burley_owen (W = H = 2^m, 2 <= m <= 12, D a power of two,
   2 D W H <= 2^32): layer k, channel pair p (0: RG, 1: BA) holds the points i = (2 k + p) W H + j, j = 0 ... W H - 1, of the
   4D Sobol sequence in plain index order: c_d = XOR of v_d[b] over the set bits b of i.  Dimension 0 is van der Corput,
   v[b] = 2^(31 - b); dimensions 1 ... 3 take Joe and Kuo's (s, a, m) = (1, 0, {1}), (2, 1, {1, 3}), (3, 1, {1, 3, 1}):
   v[b] = m_b 2^(31 - b) for b < s, else v[b] = v[b - s] ^ (v[b - s] >> s) ^ XOR over j = 1 ... s - 1 of a_j v[b - j], a_1 the
   most significant of the s - 1 bits of a.  With c'_d the scrambled coordinate, the point is written to the texel
   x = c'_0 >> (32 - m), y = c'_1 >> (32 - m): first channel of the pair c'_2 >> 16, second c'_3 >> 16.  Dimensions 0 and 1
   are a (0,2)-sequence and both scramblings keep that, so a block of W H points writes every texel exactly once.
   Scrambling, with seed_d = wang(generator_seed + 0x9E3779B9 * (d + 1)):
     sobol        c' = c (the seed is ignored)
     owen         nested uniform scrambling: bit b of c', counted from the most significant (b = 0), is bit b of c, flipped
                  iff the top bit of wang(wang((1 << b) | (c >> (32 - b))) ^ seed_d) is set (c >> 32 is 0)
     burley_owen  c' = reverse_bits(laine_karras(reverse_bits(c), seed_d)) with laine_karras(x, s): x += s;
                  x ^= x * 0x6c50b47c; x ^= x * 0xb82f1e52; x ^= x * 0xc7afe638; x ^= x * 0x8d22f6e6.  The index is not
                  shuffled: that would move points between the blocks of W H indices.

   noise_type_blue (W and H powers of two in 4 ... 128, D a power of two): channel c of layer k is the void-and-cluster
   dither array number a = 4 k + c; arrays are independent.  N = W H, n1 = N / 10 (rounded down).  Energies are float32;
   a pixel set or cleared adds or subtracts K[(y - py) mod H][(x - px) mod W] at every pixel (x, y), one operation per
   pixel, nothing contracted or reordered, where K[dy][dx] = (float) exp(-(tx^2 + ty^2) / (2 * 1.5^2)) in double with the
   toroidal distances tx = min(dx, W - dx), ty = min(dy, H - dy).  The tightest cluster is the one with the largest energy,
   the largest void the zero with the smallest; ties go to the lowest pixel index y W + x.
     1. The ones are the n1 pixels with the smallest (key, pixel), key = wang(wang(wang(generator_seed) + a) + pixel); their
        energy is added in ascending pixel order, starting from 0.
     2. Relax: the tightest cluster is removed, then the largest void is looked for.  If it is the pixel just removed, or
        this was round N, the pixel is put back (its energy added again) and the relaxation ends; otherwise the void is set.
     3. On a copy of pattern and energies, for r = n1 - 1 ... 0: the tightest cluster gets rank r and is removed.
     4. From the relaxed pattern, for r = n1 ... N / 2 - 1: the largest void gets rank r and is set.
     5. The pattern is inverted, the energy of the new ones added in ascending pixel order starting from 0; for
        r = N / 2 ... N - 1: the tightest cluster gets rank r and is removed.
   The texel is (rank * 65536 + 32768) / N, rounded down.  (At 4x4 n1 is 1 and step 2 moves the single one to pixel 0:
   all arrays of a 4x4 table are equal.) */
VKR_API int generate_noise_table(noise_table_t* noise, const device_t* device, VkExtent3D resolution,
                                 noise_type_t noise_type, uint32_t generator_seed);
/* raw RGBA16 layer-major blob, the reference's format (src/noise_table.c:96-105); path NULL: the reference's own
   file name for this type and resolution below the working directory (data/noise/..., the directories are created), so
   that load_noise_table() - and the reference itself - can read it back.  Returns 0 on success, 1 after printing one line */
VKR_API int write_noise_table(const noise_table_t* noise, noise_type_t noise_type, const char* file_path);

/* ---- noise_type_blue_noise_dithered: "a 2D blue noise dither array" (reference noise_table.h:48-51) after Georgiev and
   Fajardo, Blue-noise dithered sampling, SIGGRAPH 2016 Talks: every pixel holds a 2D sample point, arranged by swaps that
   lower an energy, so that neighbouring pixels hold distant points.  There is no reference file to match; the rule below
   is the interface and vulkan_renderer_amd/noise_tables.py restates it.  It uses integers only, so the shape of a
   parallel sum does not enter the result.  wang() and the Sobol sequence and Owen scrambling are those above; all
   integers are uint32_t unless stated.

   Resolution: W and H powers of two in 16 ... 256 with 512 <= W H <= 32768, D a power of two, 1 <= D <= 2^24;
   round_count <= 2^22.  Layer k holds two independent arrays a = 2 k + p; channels 2 p and 2 p + 1 of a texel are x and y of
   that pixel's 16-bit value.  N = W H, s = wang(wang(generator_seed) + a).

   Value set: point j (j = 0 ... N - 1) is (c'_0 >> 16, c'_1 >> 16) of point j of the Sobol sequence, Owen-scrambled with
   seed_d = wang(s + 0x9E3779B9 * (d + 1)).  Dimensions 0 and 1 are a (0,2)-sequence: the top log2(N) bits of either
   channel are a permutation of 0 ... N - 1.
   Initial assignment: pixel i = y W + x has the key wang(s + i); the pixel with the j-th smallest (key, pixel) gets point j.

   Weights, computed in double and rounded to nearest: in space, for |dx|, |dy| <= 6,
   Kq[dy][dx] = rint(65536 exp(-(dx^2 + dy^2) / 2.1^2)) with the centre set to 0; in value, for i = 0 ... 1448,
   Gq[i] = rint(65536 exp(-((i + 0.5) / 2048) / 1^2)).  Both stay below 2^16: a product fits 32 bits.  Two values are
   ax = min(|x - x'|, 65536 - |x - x'|) and ay likewise apart, r is the largest integer with r^2 <= ax^2 + ay^2, their weight
   is Gq[r >> 5].  The local energy L(p, v) of pixel p holding v is the sum over the 13x13 toroidal window around p of
   Kq[dy][dx] Gq[r(v, value of that neighbour) >> 5] as int64_t.

   Round k (k = 0 ... round_count - 1) cuts the image into 16x16 tiles, T = (W / 16) (H / 16) of them, numbered row by row.
   g = wang(wang(s ^ 0x9E3779B9) + k) moves the grid by ox = g & 15, oy = (g >> 4) & 15 and pairs the tiles by
   mask = 1 + ((((g >> 8) & 0xFFFF) (T - 1)) >> 16).  Tile t = ty (W / 16) + tx offers the pixel
   ((16 tx + ox + cx) mod W, (16 ty + oy + cy) mod H) with h = wang(wang(s + k) + t), cx = ((h & 0xFFFF) 10) >> 16,
   cy = ((h >> 16) 10) >> 16.  For every pair (t, t ^ mask) with t < t ^ mask, with p and q their pixels holding v_p and v_q:
   delta = L(p, v_q) + L(q, v_p) - L(p, v_p) - L(q, v_q), and the two values are exchanged iff delta < 0.  The pixels of a
   round lie in the 10x10 cores of their tiles, more than 6 apart on the torus: no window holds another pixel of the
   round, the swaps of a round do not see each other, and the sum of all local energies never rises.  n rounds are the
   first n rounds of any longer run.

   generate_dithered_noise_table() follows the conventions of generate_noise_table(): device_data by HIP kernels on
   device->stream (at most VKR_DITHERED_ROUNDS_PER_LAUNCH rounds per launch; the table itself is the state between
   launches), host_data by one read-back, random_seed = 3124705, 0 on success; 1 after printing one line, with the struct
   zeroed, for device == NULL, a resolution outside the range and more than 2^22 rounds. */
#define VKR_DITHERED_ROUNDS_PER_LAUNCH 4096
VKR_API int generate_dithered_noise_table(noise_table_t* noise, const device_t* device, VkExtent3D resolution,
                                          uint32_t generator_seed, uint32_t round_count);
/* 2^19 for every resolution: the round count beyond which twice the rounds raise the mean distance between the values of
   neighbouring pixels by less than 1 % (which also says why a renderer is served better by about 2^10) */
VKR_API uint32_t get_default_dithered_round_count(VkExtent3D resolution);
/* Kq, row by row from dy = -6, and Gq as the generator uses them */
VKR_API void get_dithered_noise_weights(uint32_t spatial[169], uint32_t value[1449]);

#endif
