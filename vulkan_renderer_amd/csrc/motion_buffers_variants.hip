// The motion images of a frame (include/vkr_motion_buffers.h): the barycentrics of the pixel ray on the triangle as it is,
// applied to the triangle's vertices as they were, and that point under the previous frame's matrix.  Starts from
// shading_inputs.h alone, as the feature images do; no material and no texture sampler.  Built once per arithmetic mode: in
// the libm and the polynomial mode the images equal vulkan_renderer_amd/motion_buffers.py in every bit.
#include "shading_inputs.h"
#include "shade_launchers.h"  // (the declaration that the caller of the launcher below sees)

#if VKR_FAST_MATH
#define VKR_MOTION_LAUNCH_NAME vkr_launch_motion_buffers_fast
#elif VKR_MATH_MODE == 2
#define VKR_MOTION_LAUNCH_NAME vkr_launch_motion_buffers_libm
#else
#define VKR_MOTION_LAUNCH_NAME vkr_launch_motion_buffers_exact
#endif

using namespace vkr;

inline namespace VKR_MODE_NAMESPACE {

// the positions of the previous frame, where the images go (NULL: not wanted; wave-uniform) and the three rows of the
// previous frame's matrix that are used
struct motion_targets {
	const uint2* previous_positions;
	float4 *reprojection, *previous_position, *motion;
	float row_x[4], row_y[4], row_w[4];
};

// c_i of include/vkr_motion_buffers.h: every operation rounded on its own in the IEEE modes
VKR_DEV float project_row(const float (&row)[4], f3 position) {
	return ((row[0] * position.x + row[1] * position.y) + row[2] * position.z) + row[3];
}

// One lane per pixel, 16x16 pixels per workgroup, 8x8 per wave (the mapping of k_feature_buffers), one 16-byte store per
// wanted image.  The three previous vertices are requested in front of intersect_primitive(), whose three loads of the
// current ones follow at once: six loads in flight before any arithmetic (its loads of normals and texture coordinates
// have no user here and are not made).  A wave without a covered pixel only stores.
__global__ void __launch_bounds__(256) k_motion_buffers(const shade_params p, const motion_targets t) {
	uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	uint32_t px = blockIdx.x * 16 + ((wave & 1) << 3) + (lane & 7);
	uint32_t py = blockIdx.y * 16 + ((wave >> 1) << 3) + (lane >> 3);
	if (px >= p.width || py >= p.height) return;
	size_t pixel = (size_t) py * p.width + px;
	uint32_t primitive = p.visibility[pixel];
	// a pixel with nothing visible: sixteen zero bytes in every image
	const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	float4 reprojection = zero, previous_position = zero, motion = zero;
	if (primitive != 0xFFFFFFFFu) {
		const uint8_t* c = p.constants;
		uint2 old_words[3];
#pragma unroll
		for (int i = 0; i < 3; ++i) old_words[i] = t.previous_positions[(size_t) primitive * 3 + i];
		float fx = (float) (int32_t) px, fy = (float) (int32_t) py;
		f3 ray = mk3(
			(load_f(c, 96) * fx + load_f(c, 100) * fy) + load_f(c, 104) * 1.0f,
			(load_f(c, 112) * fx + load_f(c, 116) * fy) + load_f(c, 120) * 1.0f,
			(load_f(c, 128) * fx + load_f(c, 132) * fy) + load_f(c, 136) * 1.0f);
		triangle_hit hit = intersect_primitive(p, primitive, ray);
		f3 factor = load_f3(c, 0), summand = load_f3(c, 16);
		f3 old0 = decode_position(old_words[0], factor, summand), old1 = decode_position(old_words[1], factor, summand), old2 = decode_position(old_words[2], factor, summand);
		f3 P = fma3(hit.b0, hit.pos[0], fma3(hit.b1, hit.pos[1], hit.pos[2] * hit.b2));
		f3 Q = fma3(hit.b0, old0, fma3(hit.b1, old1, old2 * hit.b2));
		float c_x = project_row(t.row_x, Q), c_y = project_row(t.row_y, Q), c_w = project_row(t.row_w, Q);
		float width = (float) p.width, height = (float) p.height;
		float x = (divide(c_x, c_w) + 1.0f) * (0.5f * width) - 0.5f;
		float y = (divide(c_y, c_w) + 1.0f) * (0.5f * height) - 0.5f;
		// (every comparison fails for a NaN)
		float inside = (c_w > 0.0f && x >= -0.5f && x < width - 0.5f && y >= -0.5f && y < height - 0.5f) ? 1.0f : 0.0f;
		f3 d = Q - P;
		reprojection = make_float4(x, y, c_w, inside);
		previous_position = make_float4(Q.x, Q.y, Q.z, 1.0f);
		motion = make_float4(x - fx, y - fy, square_root((d.x * d.x + d.y * d.y) + d.z * d.z), inside);
	}
	if (t.reprojection) t.reprojection[pixel] = reprojection;
	if (t.previous_position) t.previous_position[pixel] = previous_position;
	if (t.motion) t.motion[pixel] = motion;
}

}  // inline namespace VKR_MODE_NAMESPACE

// images: reprojection, previous_position, motion
extern "C" int VKR_MOTION_LAUNCH_NAME(const shade_params* p, const void* previous_positions, void* const* images, const float* previous_matrix, void* stream) {
	motion_targets t;
	t.previous_positions = (const uint2*) previous_positions;
	t.reprojection = (float4*) images[0]; t.previous_position = (float4*) images[1]; t.motion = (float4*) images[2];
	for (int j = 0; j != 4; ++j) {
		t.row_x[j] = previous_matrix[j]; t.row_y[j] = previous_matrix[4 + j]; t.row_w[j] = previous_matrix[12 + j];
	}
	dim3 grid((p->width + 15) / 16, (p->height + 15) / 16);
	k_motion_buffers<<<grid, 256, 0, (hipStream_t) stream>>>(*p, t);
	return hipGetLastError() != hipSuccess;
}
