/* Conversion of images to *.vkt textures on the device: reference tools/texture_conversion/main.c:105-405. */
#ifndef VKR_TEXTURE_CONVERSION_H
#define VKR_TEXTURE_CONVERSION_H
#include "vkr_device.h"

/*! The formats of reference main.c:31-39 and the two 8-bit formats that the loaders read as well (csrc/host/textures.c) */
typedef enum texture_conversion_format_e {
	texture_conversion_format_r8g8b8a8_unorm = 37,
	texture_conversion_format_r8g8b8a8_srgb = 43,
	texture_conversion_format_r16g16b16_sfloat = 90,
	texture_conversion_format_r16g16b16a16_sfloat = 97,
	texture_conversion_format_r32g32b32_sfloat = 106,
	texture_conversion_format_r32g32b32a32_sfloat = 109,
	texture_conversion_format_bc1_rgb_unorm = 131,
	texture_conversion_format_bc1_rgb_srgb = 132,
	texture_conversion_format_bc5_unorm = 141,
} texture_conversion_format_t;

/*! What reference main.c:43-65 writes in front of the payload, and the payload */
typedef struct converted_texture_s {
	/*! The VkFormat, the number of levels and the extent of level 0 */
	int32_t format, mipmap_count, width, height;
	/*! Bytes of all levels, of each level, and where each level begins in the payload */
	uint64_t payload_size, mipmap_sizes[32], mipmap_offsets[32];
	/*! Host memory, all levels, largest first */
	uint8_t* payload;
} converted_texture_t;

/* convert_texture() converts a row-major image with channel_count interleaved channels on the device (HIP kernels of
   csrc/texture_conversion.hip on device->stream: one upload of the source, one of the tables and filter weights, one device
   buffer for the payload, one read-back) and returns 0.  The four float formats take float pixels, all others uint8_t;
   channels beyond the format's (2 for 141, 3 for 90, 106, 131, 132, 4 for 37, 43, 97, 109) are dropped.  It returns 1 after
   printing one line, with the struct zeroed, for: device == NULL (there is no host build of the converter), an unknown
   format, too few channels, an extent that is not a power of two or is above 4096 (the filter weights of the top level
   stay within the 64 KiB of LDS a workgroup has by default), and a block format below 4x4 - except 1x1, which becomes one
   constant 4x4 level (main.c:243-255).  The rules that follow, the order of operations included, are the interface: the
   numpy restatement vulkan_renderer_amd/texture_conversion.py gives the same bytes.  Up to the quantised texels they are
   the reference tool's, operation for operation; binary32 throughout, nothing contracted or reordered.

   Levels (main.c:93-102, 229-261, 278-291).  The count is min(log2 W, log2 H) + 1, two less for the block formats (their
   smallest level is four texels along its shorter axis); level i is (W >> i) x (H >> i) and follows level i - 1 in the
   payload without padding.

   Linear image (main.c:85-88, 205-215).  Floats pass through.  Bytes become b * (1 / 255.f), bytes of the colour channels
   of the two sRGB formats s = b * (1 / 255.f); s <= 0.04045f ? s * (1 / 12.92f) : powf(s * (1 / 1.055f) + 0.055f / 1.055f,
   2.4f), by a table of 256 entries made on the host.  Alpha of format 43 is linear (this project's rule: the tool has no
   four-channel sRGB format).  powf is glibc 2.35's, restated in csrc/glibc_math.h, here and below: neither the libm of
   the host nor the device's enters a byte.

   Levels above 0 (main.c:306-343) are each filtered from the linear level 0, not from the level below.  stride = 2^i,
   sigma = 0.4f * stride, E = (int) ceilf(3.0f * sigma), g = -0.5f / (sigma * sigma), c = E - 0.5f.  The 2 E weights are
   w[j] = (float) exp((double) a) with a = (g * (j - c)) * (j - c) formed in binary32; their sum is taken in binary32 in
   ascending j and every weight multiplied by 1.0f / sum.  (The tool calls expf(a).  Over the levels 1 ... 12 of extents
   up to 4096 glibc 2.35's expf gives other bits for 14 of the 19668 weights, eight of level 11 and six of level 12, by one
   unit in the last place; for those the rule is the bits expf gave, listed in csrc/host/texture_conversion.c and in the
   restatement.  The fixtures of tests/golden/texture_conversion.npz reach level 5.)  A texel channel starts from +0.0f and adds (w[j] * w[k]) * source in the order
   k (rows) outer, j (columns) inner, k, j = 0 ... 2 E - 1, the source texel being ((x * stride + stride / 2 - E + j) &
   (W - 1), (y * stride + stride / 2 - E + k) & (H - 1)).  The chain of additions is sequential: that is what byte parity
   with the tool costs.

   Float formats (main.c:383-394).  106 and 109 store the floats.  90 and 97 store halves by the tool's float_to_half: the
   sign is set aside; NaN becomes 0x7E00 and infinity 0x7C00; otherwise the low 12 bits of the binary32 pattern are cleared,
   the value is multiplied by 2^-112 in binary32 (exact for normal results; a result below 2^-126, that is a half
   subnormal, is rounded to nearest even there), 0x1000 is added to the pattern, a pattern above 0x0F800000 (infinity of
   the half) becomes that, and the pattern shifted right by 13 is the half.  Up to the half subnormals this rounds to
   nearest by looking at the first dropped bit only: ties go away from zero, not to even.

   Quantisation to 8 bits (main.c:70-80).  UNORM: roundf(v * 255.0f).  sRGB colour channels: v = v < 0 ? 0 : v; s =
   v <= 0.0031308f ? 12.92f * v : 1.055f * powf(v, 1.0f / 2.4f) - 0.055f; roundf(s * 255.0f).  The result is clamped to
   0 ... 255 (no clamp is ever taken with byte inputs: the weights are positive and normalised).  Block (bx, by) of a level
   holds the texels (4 bx + x, 4 by + y) as texel number 4 y + x; blocks are stored row by row.

   BC5 (format 141) is two BC4 blocks, red then green.  With min and max the extremes of the 16 values, the candidate pairs
   are every (hi, lo) with hi in [max(min, max - 4), max] and lo in [min, min(max, min + 4)], each as (e0, e1) = (hi, lo)
   and as (lo, hi).  The palette is the one of decode_bc4_block (csrc/host/textures.c): e0, e1, then for e0 > e1
   ((7 - i) e0 + i e1 + 3) / 7, i = 1 ... 6, else ((5 - i) e0 + i e1 + 2) / 5, i = 1 ... 4, 0 and 255.  Each texel takes
   the entry of least squared difference, ties to the lowest index; the error of a pair is the integer sum over the texels.
   The pair of least error wins, ties to the lowest (e0 << 8) | e1.  (max, min), the choice of synthetic.encode_bc4 and
   of stb_dxt, is among the candidates; a constant block comes out as (v, v) with all indices 0.  Index i of texel t is
   stored at bit 3 t of the 48 bits behind the endpoints.

   BC1 (formats 131, 132).  The state is e = (r0, g0, b0, r1, g1, b1) in 5 / 6 / 5 bits.  E(e): c = (r << 11) | (g << 5) | b
   of both colours, swapped if c0 < c1; the palette of vkr_decode_bc1_block (endpoints expanded by bit replication,
   (2 a + b + 1) / 3 and (a + 2 b + 1) / 3); each texel takes the entry of least squared difference summed over R, G, B,
   ties to the lowest index (so all indices are 0 for c0 == c1); E is the integer sum over the texels.  Three start states:
     A  the texels of largest and of smallest 2 R + 5 G + B, ties to the lowest texel number, truncated to 5 / 6 / 5 bits
        (r >> 3, g >> 2, b >> 3): the endpoints of synthetic.encode_bc1.
     B  the ends of the principal axis, in 64-bit integers.  With S_a the sum of channel a over the texels and P_ab the sum
        of products, C_ab = 16 P_ab - S_a S_b.  v is the row of C with the largest diagonal entry (ties to the first),
        normalised; four times v = C v, normalised.  Normalising shifts every component right (arithmetically) by
        max(0, n - 10), n the bit length of the largest magnitude.  The texels of largest and of smallest v . t, ties to
        the lowest texel number, rounded to nearest: r5 = (31 r + 127) / 255, g6 = (63 g + 127) / 255, b like r.
     C  the corners (max R, max G, max B) and (min R, min G, min B) of the bounding box, rounded to nearest as in B.
   From each start state rounds of trials run: a round changes component k by s for k = 0 ... 5 (outer) and s = -1, +1
   (inner), then for k = 0 ... 5 and s = -2, +2 (steps of one alone leave one level of the fixtures' images behind
   stb_dxt); a trial that stays in range and has a strictly lower E is accepted at once and the round goes on from it.
   The descent ends after a round without acceptance or after 32 rounds.  The state of lowest E wins, ties to the earlier start state.  The
   block stores c0, c1 (after the swap) as two little-endian uint16_t and the index of texel t at bit 2 t of the uint32_t
   behind them.  No state is worse than A, so no block is worse than synthetic.encode_bc1's. */
VKR_API int convert_texture(converted_texture_t* out, const device_t* device, const void* pixels,
                            uint32_t width, uint32_t height, uint32_t channel_count, int32_t vk_format);
/*! The container of reference src/textures.c:95-129 as main.c:271-291, 398-399 writes it: six int32_t (0xbc1bc1, 1, count,
	width, height, format), the uint64_t payload size, per level int32_t width and height, uint64_t size and offset, the
	payload, uint32_t 0xE0FE0F.  Returns 0 on success, 1 after printing one line */
VKR_API int write_converted_texture(const converted_texture_t* texture, const char* file_path);
VKR_API void free_converted_texture(converted_texture_t* texture);

/*! What the rules above take from the host, for restatements in other languages: out[i] = powf(x[i], y) of
	csrc/glibc_math.h, the two tables of 256 floats the bytes of an image go through (tables[b]: the sRGB curve of the
	linear image above, tables[256 + b] = b * (1 / 255.f)), and the normalised weights of level `level`: returns E, or 0 for levels outside 1 ... 12, and
	writes the first min(2 E, capacity) weights if weights is not NULL */
VKR_API void evaluate_texture_conversion_powf(float* out, const float* x, float y, uint64_t count);
VKR_API void get_texture_conversion_tables(float tables[512]);
VKR_API uint32_t get_texture_filter_weights(float* weights, uint32_t capacity, uint32_t level);

#endif
