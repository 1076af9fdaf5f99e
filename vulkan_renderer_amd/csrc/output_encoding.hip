// Output encoding (shading_pass.frag.glsl:871-892, srgb_utility.glsl): radiance -> RGBA8 or packed RGB8, of the
// frame or of a slab.  The table of sRGB code starts is a __device__ global; the library is built without relocatable
// device code, so the table, the kernel that fills it and every kernel that reads it live in this one unit.
// Compiled in exact mode (-ffp-contract=off): srgb_code_by_powf restates the oracle operation for operation.
#include "pass_internal.h"
#include "device_math.h"  // gclamp, gm_powf, divide
#include "vkr_feature_buffers.h"  // pixel_feature_t of k_feature_preview
#include <hip/hip_fp16.h>

using namespace vkr;

__device__ __forceinline__ float linear_to_srgb(float v) {
	v = gclamp(v, 0.0f, 1.0f);
	return (v <= 0.0031308f) ? (12.92f * v) : (1.055f * powf(v, 1.0f / 2.4f) - 0.055f);
}
__device__ __forceinline__ float srgb_to_linear(float v) {
	v = gclamp(v, 0.0f, 1.0f);
	return (v <= 0.04045f) ? ((1.0f / 12.92f) * v) : powf(fmaf(v, 1.0f / 1.055f, 0.055f / 1.055f), 2.4f);
}
__device__ __forceinline__ uint32_t to_unorm8(float v) {
	v = gclamp(v, 0.0f, 1.0f);
	return (uint32_t) (v * 255.0f + 0.5f);
}

// to_unorm8(linear_to_srgb(v)) without the pow: the code is the number of starts T[c], c = 1 ... 255, that v has
// reached, where T[c] is the first float whose code is c in the oracle's float arithmetic (oracle_srgb8_code_starts:
// gm_powf, no contraction, a code that never decreases over [0, 1]).  The starts lie up to 4 ulps away from the
// exact thresholds srgb_to_linear((c - 0.5) / 255), on either side, at 171 of the 255 codes.  A hardware log2 / exp2
// estimate is off by less than one code; the two neighbouring starts settle it.
// (Three powf per pixel made the encode kernel as expensive as tracing config 2's shadow rays.)
__device__ float g_srgb_code_thresholds[257];

// the oracle's to_unorm8(linear_to_srgb(v)) for v in [0, 1], operation for operation (this file: -ffp-contract=off)
__device__ uint32_t srgb_code_by_powf(float v) {
	float s = (v <= 0.0031308f) ? (12.92f * v) : (1.055f * gm_powf(v, 1.0f / 2.4f) - 0.055f);
	s = gclamp(s, 0.0f, 1.0f);
	return (uint32_t) (s * 255.0f + 0.5f);
}

// thread c bisects the float bit patterns of [0, 1] for the start of code c (30 steps of one powf)
__global__ void k_fill_srgb_code_thresholds() {
	uint32_t c = threadIdx.x;
	uint32_t below = 0u, start = 0x3F800000u;  // code(below) < c <= code(start)
	while (c != 0 && start - below > 1u) {
		uint32_t middle = below + (start - below) / 2u;
		if (srgb_code_by_powf(__uint_as_float(middle)) >= c) start = middle;
		else below = middle;
	}
	g_srgb_code_thresholds[c] = (c == 0) ? 0.0f : __uint_as_float(start);
	if (c == 0) g_srgb_code_thresholds[256] = __builtin_inff();
}

// Called by create_hip_device() with the device selected: fills the table on THAT device and waits, so that
// every stream of every thread that later encodes on the device finds it (the table is per device and its
// content does not depend on who fills it: no host-side state, filling it again is harmless).
extern "C" int vkr_fill_device_tables(void* stream) {
	k_fill_srgb_code_thresholds<<<1, 256, 0, (hipStream_t) stream>>>();
	if (hip_failed(hipGetLastError(), "filling the sRGB code starts")) return 1;
	return hip_failed(hipStreamSynchronize((hipStream_t) stream), "filling the sRGB code starts");
}

// The other thing device.c needs from a HIP unit: the kernel that warms a stream up
static __global__ void k_empty() {}
extern "C" int vkr_launch_empty_kernel(void* stream) {
	k_empty<<<1, 64, 0, (hipStream_t) stream>>>();
	return hipGetLastError() != hipSuccess;
}

__device__ __forceinline__ uint32_t srgb_code(float v) {
	v = gclamp(v, 0.0f, 1.0f);  // (NaN -> 0 like to_unorm8(linear_to_srgb(NaN)))
	float estimate = (v <= 0.0031308f) ? (12.92f * v) : fmaf(1.055f, __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(v) * (1.0f / 2.4f)), -0.055f);
	uint32_t c = (uint32_t) fmaf(gclamp(estimate, 0.0f, 1.0f), 255.0f, 0.5f);
	c = (v < g_srgb_code_thresholds[c]) ? c - 1u : c;
	c = (v >= g_srgb_code_thresholds[c + 1u]) ? c + 1u : c;
	return c;
}

// packHalf2x16 of one channel.  Which NaN a NaN becomes is left to the implementation by the reference; it is pinned
// to the oracle's sign | 0x7E00 here (v_cvt_f16_f32 keeps the payload's upper bits).
__device__ __forceinline__ uint32_t half_bits(float x) {
	uint32_t h = __half_as_ushort(__float2half_rn(x));
	return (x != x) ? (((__float_as_uint(x) >> 16) & 0x8000u) | 0x7E00u) : h;
}

__device__ __forceinline__ uint32_t encode_pixel(float4 c, uint32_t frame_bits, int output_linear_rgb) {
	uint32_t r, g, b, a;
	if (frame_bits == 0) {
		// an *_SRGB target encodes in hardware, any other gets the transfer function in the shader
		r = srgb_code(c.x); g = srgb_code(c.y); b = srgb_code(c.z);
		a = to_unorm8(c.w);
	}
	else {
		uint32_t mask = (frame_bits == 1) ? 0xFF : 0xFF00, shift = (frame_bits == 1) ? 0 : 8;
		uint32_t h0 = half_bits(c.x) | (half_bits(c.y) << 16);
		uint32_t h1 = half_bits(c.z);
		float v[3] = {
			(float) ((h0 & mask) >> shift) * (1.0f / 255.0f),
			(float) ((((h0 & 0xFFFF0000u) >> 16) & mask) >> shift) * (1.0f / 255.0f),
			(float) ((h1 & mask) >> shift) * (1.0f / 255.0f)};
		uint32_t out[3];
		for (int j = 0; j != 3; ++j) out[j] = to_unorm8(output_linear_rgb ? linear_to_srgb(srgb_to_linear(v[j])) : v[j]);
		r = out[0]; g = out[1]; b = out[2];
		a = 255;
	}
	return r | (g << 8) | (b << 16) | (a << 24);
}

__global__ void __launch_bounds__(256) k_encode_output(const float4* radiance, uint32_t* encoded, uint64_t pixel_count, uint32_t frame_bits, int output_linear_rgb) {
	uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= pixel_count) return;
	encoded[i] = encode_pixel(radiance[i], frame_bits, output_linear_rgb);
}

// four pixels per thread: twelve bytes of packed RGB as three dwords
__global__ void __launch_bounds__(256) k_encode_output_rgb8(const float4* radiance, uint32_t* packed, uint64_t quad_count, uint32_t frame_bits, int output_linear_rgb) {
	uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= quad_count) return;
	uint32_t p0 = encode_pixel(radiance[4 * i], frame_bits, output_linear_rgb) & 0xFFFFFFu, p1 = encode_pixel(radiance[4 * i + 1], frame_bits, output_linear_rgb) & 0xFFFFFFu;
	uint32_t p2 = encode_pixel(radiance[4 * i + 2], frame_bits, output_linear_rgb) & 0xFFFFFFu, p3 = encode_pixel(radiance[4 * i + 3], frame_bits, output_linear_rgb) & 0xFFFFFFu;
	packed[3 * i] = p0 | (p1 << 24);
	packed[3 * i + 1] = (p1 >> 8) | (p2 << 16);
	packed[3 * i + 2] = (p2 >> 16) | (p3 << 8);
}

static void launch_encode(const void* radiance, void* encoded, uint64_t pixel_count, uint32_t frame_bits, int output_linear_rgb, hipStream_t stream) {
	k_encode_output<<<(uint32_t) ((pixel_count + 255) / 256), 256, 0, stream>>>((const float4*) radiance, (uint32_t*) encoded, pixel_count, frame_bits, output_linear_rgb);
}

void launch_encode_rgb8(const void* radiance, void* packed, uint64_t pixel_count, uint32_t frame_bits, int output_linear_rgb, hipStream_t stream) {
	k_encode_output_rgb8<<<(uint32_t) ((pixel_count / 4 + 255) / 256), 256, 0, stream>>>((const float4*) radiance, (uint32_t*) packed, pixel_count / 4, frame_bits, output_linear_rgb);
}

// The previews of the feature images (include/vkr_feature_buffers.h "Previews"): one lane per pixel, integer and binary32
// only, nothing contracted; vulkan_renderer_amd/feature_buffers.py restates every line in numpy.
// u8() of the header: the clamp spelled out so that a NaN gives 0 by a comparison, not by the conversion
__device__ __forceinline__ uint32_t preview_unorm8(float v) {
	v = (v > 0.0f) ? gmin(v, 1.0f) : 0.0f;
	return (uint32_t) (v * 255.0f + 0.5f);
}

__global__ void __launch_bounds__(256) k_feature_preview(uint32_t feature, const uint4* image, uint32_t* out_rgba8, uint32_t width, uint32_t height, float range_low, float range_high) {
	uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= (uint64_t) width * height) return;
	const uint4 bits = image[i];
	const float x = __uint_as_float(bits.x), y = __uint_as_float(bits.y), z = __uint_as_float(bits.z), w = __uint_as_float(bits.w);
	uint32_t r, g, b;
	switch (feature) {
	case pixel_feature_normal: case pixel_feature_outgoing:
		r = preview_unorm8(x * 0.5f + 0.5f); g = preview_unorm8(y * 0.5f + 0.5f); b = preview_unorm8(z * 0.5f + 0.5f);
		break;
	case pixel_feature_diffuse_albedo: case pixel_feature_fresnel_0:
		r = srgb_code(x); g = srgb_code(y); b = srgb_code(z);
		break;
	case pixel_feature_position:
		r = g = b = preview_unorm8(divide(w - range_low, range_high - range_low));
		break;
	case pixel_feature_reprojection: {
		float px = (float) (uint32_t) (i % width), py = (float) (uint32_t) (i / width);
		r = preview_unorm8(divide((x - px) + range_high, 2.0f * range_high));
		g = preview_unorm8(divide((y - py) + range_high, 2.0f * range_high));
		b = preview_unorm8(w);
		break;
	}
	default: {  // pixel_feature_identity
		uint32_t h = bits.x * 2654435761u;
		if (bits.x == 0xFFFFFFFFu) h = 0u;
		r = h & 255u; g = (h >> 8) & 255u; b = (h >> 16) & 255u;
		break;
	}
	}
	out_rgba8[i] = r | (g << 8) | (b << 16) | 0xFF000000u;
}

void launch_feature_preview(uint32_t feature, const void* image, void* out_rgba8, uint32_t width, uint32_t height, float range_low, float range_high, hipStream_t stream) {
	uint64_t pixel_count = (uint64_t) width * height;
	k_feature_preview<<<(uint32_t) ((pixel_count + 255) / 256), 256, 0, stream>>>(feature, (const uint4*) image, (uint32_t*) out_rgba8, width, height, range_low, range_high);
}

extern "C" int encode_output(application_t* app, VkBool32 output_linear_rgb) {
	if (finish_frames(app)) return 1;
	uint64_t pixels = (uint64_t) app->swapchain.extent.width * app->swapchain.extent.height;
	if (!app->render_targets.radiance || !app->render_targets.encoded) return 1;
	launch_encode(app->render_targets.radiance, app->render_targets.encoded, pixels, app->screenshot.frame_bits, output_linear_rgb ? 1 : 0, (hipStream_t) app->device.stream);
	note_target_reader(app);
	return hip_failed(hipGetLastError(), "encoding the output");
}

extern "C" int encode_slab(application_t* app, const void* slab_radiance, void* slab_encoded, uint64_t pixel_count, VkBool32 output_linear_rgb) {
	if (finish_frames(app)) return 1;
	if (!slab_radiance || !slab_encoded) return 1;
	launch_encode(slab_radiance, slab_encoded, pixel_count, app->screenshot.frame_bits, output_linear_rgb ? 1 : 0, (hipStream_t) app->device.stream);
	note_target_reader(app);
	return hip_failed(hipGetLastError(), "encoding the slab");
}

extern "C" int encode_slab_rgb8(application_t* app, const void* slab_radiance, void* slab_rgb8, uint64_t pixel_count, VkBool32 output_linear_rgb) {
	if (finish_frames(app)) return 1;
	if (!slab_radiance || !slab_rgb8 || pixel_count % 4 != 0) {
		printf("encode_slab_rgb8() needs buffers and a pixel count that is a multiple of four (slabs are).\n");
		return 1;
	}
	launch_encode_rgb8(slab_radiance, slab_rgb8, pixel_count, app->screenshot.frame_bits, output_linear_rgb ? 1 : 0, (hipStream_t) app->device.stream);
	note_target_reader(app);
	return hip_failed(hipGetLastError(), "encoding the slab");
}
