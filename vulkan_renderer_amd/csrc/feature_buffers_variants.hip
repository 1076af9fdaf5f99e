// The feature images of a frame (include/vkr_feature_buffers.h): what get_shading_data() yields for every pixel, written
// out instead of shaded.  Starts from shading_inputs.h alone - nothing of the shading program is compiled here.
// Built once per arithmetic mode: the images of the libm and of the polynomial mode equal oracle_shading_data() in
// math mode 0 and 1, in every bit.
#include "shading_inputs.h"
#include "shade_launchers.h"  // (the declaration that the caller of the launcher below sees)

#if VKR_FAST_MATH
#define VKR_FEATURE_LAUNCH_NAME vkr_launch_feature_buffers_fast
#elif VKR_MATH_MODE == 2
#define VKR_FEATURE_LAUNCH_NAME vkr_launch_feature_buffers_libm
#else
#define VKR_FEATURE_LAUNCH_NAME vkr_launch_feature_buffers_exact
#endif

using namespace vkr;

inline namespace VKR_MODE_NAMESPACE {

// where the images go (NULL: not wanted; wave-uniform) and the three rows of the reprojection matrix that are used
struct feature_targets {
	float4 *position, *normal, *outgoing, *diffuse_albedo, *fresnel_0;
	uint4* identity;
	float4* reprojection;
	float row_x[4], row_y[4], row_w[4];
};

// c_i of include/vkr_feature_buffers.h: every operation rounded on its own in the IEEE modes
VKR_DEV float project_row(const float (&row)[4], f3 position) {
	return ((row[0] * position.x + row[1] * position.y) + row[2] * position.z) + row[3];
}

// One lane per pixel, 16x16 pixels per workgroup, 8x8 per wave (the mapping of k_resolve_materials): one
// get_shading_data() per covered pixel, then one 16-byte store per wanted image.  A wave without a covered pixel only
// stores.  TEXTURED: the material comes from resolve_material(), evaluated here; the other instantiation carries no sampler.
template <bool TEXTURED>
__global__ void __launch_bounds__(256) k_feature_buffers(const shade_params p, const feature_targets t) {
	uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	uint32_t px = blockIdx.x * 16 + ((wave & 1) << 3) + (lane & 7);
	uint32_t py = blockIdx.y * 16 + ((wave >> 1) << 3) + (lane >> 3);
	if (px >= p.width || py >= p.height) return;
	size_t pixel = (size_t) py * p.width + px;
	uint32_t primitive = p.visibility[pixel];
	// a pixel with nothing visible: sixteen zero bytes in every float image
	const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	float4 position = zero, normal = zero, outgoing = zero, diffuse_albedo = zero, fresnel_0 = zero, reprojection = zero;
	uint32_t material = 0xFFFFFFFFu;
	if (primitive != 0xFFFFFFFFu) material = p.material_indices[primitive];
	// (the identity image alone needs no shading point)
	const bool shading_point_wanted = t.position || t.normal || t.outgoing || t.diffuse_albedo || t.fresnel_0 || t.reprojection;
	if (primitive != 0xFFFFFFFFu && shading_point_wanted) {
		const uint8_t* c = p.constants;
		float fx = (float) (int32_t) px, fy = (float) (int32_t) py;
		f3 ray = mk3(
			(load_f(c, 96) * fx + load_f(c, 100) * fy) + load_f(c, 104) * 1.0f,
			(load_f(c, 112) * fx + load_f(c, 116) * fy) + load_f(c, 120) * 1.0f,
			(load_f(c, 128) * fx + load_f(c, 132) * fy) + load_f(c, 136) * 1.0f);
		shading_data s;
		if constexpr (TEXTURED) {
			// the lane's own material, resolved here, handed to get_shading_data() as a material buffer of one pixel (the
			// array stays in registers: scratch is 0)
			float values[8];
			resolve_material(p, primitive, ray, values);
			shade_params own = p;
			own.pixel_materials = values;
			s = get_shading_data(own, primitive, ray, 0);
		}
		else
			s = get_shading_data(p, primitive, ray, 0);  // (p.pixel_materials is NULL: the constant material)
		f3 d = load_f3(c, 144) - s.position;
		float distance = square_root((d.x * d.x + d.y * d.y) + d.z * d.z);
		position = make_float4(s.position.x, s.position.y, s.position.z, distance);
		normal = make_float4(s.normal.x, s.normal.y, s.normal.z, s.lambert_outgoing);
		outgoing = make_float4(s.outgoing.x, s.outgoing.y, s.outgoing.z, 1.0f);
		diffuse_albedo = make_float4(s.diffuse_albedo.x, s.diffuse_albedo.y, s.diffuse_albedo.z, s.roughness);
		fresnel_0 = make_float4(s.fresnel_0.x, s.fresnel_0.y, s.fresnel_0.z, 1.0f);
		if (t.reprojection) {
			float c_x = project_row(t.row_x, s.position), c_y = project_row(t.row_y, s.position), c_w = project_row(t.row_w, s.position);
			float width = (float) p.width, height = (float) p.height;
			float x = (divide(c_x, c_w) + 1.0f) * (0.5f * width) - 0.5f;
			float y = (divide(c_y, c_w) + 1.0f) * (0.5f * height) - 0.5f;
			// (every comparison fails for a NaN)
			bool inside = c_w > 0.0f && x >= -0.5f && x < width - 0.5f && y >= -0.5f && y < height - 0.5f;
			reprojection = make_float4(x, y, c_w, inside ? 1.0f : 0.0f);
		}
	}
	if (t.position) t.position[pixel] = position;
	if (t.normal) t.normal[pixel] = normal;
	if (t.outgoing) t.outgoing[pixel] = outgoing;
	if (t.diffuse_albedo) t.diffuse_albedo[pixel] = diffuse_albedo;
	if (t.fresnel_0) t.fresnel_0[pixel] = fresnel_0;
	if (t.identity) t.identity[pixel] = make_uint4(primitive, material, px, py);
	if (t.reprojection) t.reprojection[pixel] = reprojection;
}

}  // inline namespace VKR_MODE_NAMESPACE

// images: pixel_feature_count pointers in the order of pixel_feature_t
extern "C" int VKR_FEATURE_LAUNCH_NAME(const shade_params* p, void* const* images, const float* reprojection, int textured, void* stream) {
	feature_targets t;
	t.position = (float4*) images[0]; t.normal = (float4*) images[1]; t.outgoing = (float4*) images[2];
	t.diffuse_albedo = (float4*) images[3]; t.fresnel_0 = (float4*) images[4];
	t.identity = (uint4*) images[5];
	t.reprojection = (float4*) images[6];
	for (int j = 0; j != 4; ++j) {
		t.row_x[j] = reprojection[j]; t.row_y[j] = reprojection[4 + j]; t.row_w[j] = reprojection[12 + j];
	}
	dim3 grid((p->width + 15) / 16, (p->height + 15) / 16);
	if (textured) k_feature_buffers<true><<<grid, 256, 0, (hipStream_t) stream>>>(*p, t);
	else k_feature_buffers<false><<<grid, 256, 0, (hipStream_t) stream>>>(*p, t);
	return hipGetLastError() != hipSuccess;
}
