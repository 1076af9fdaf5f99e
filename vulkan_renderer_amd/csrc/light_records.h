// The packed light records of the constant buffer (include/vkr_polygonal_light.h), the ray test against a light's
// polygon, and the radiance of a light with its texture.
//
// Follows reference src/shaders/polygonal_light_utility.glsl:93-112 (polygonal_light_ray_intersection) and
// src/shaders/shading_pass.frag.glsl:151-185 (get_polygon_radiance); the light texture sampler is that of reference
// src/main.c:611-621.
#pragma once
#include "shading_inputs.h"

namespace vkr {

// ---- lights ----------------------------------------------------------------------

// Wave-uniform view of one packed light record (include/vkr_polygonal_light.h)
struct light_ref {
	const uint8_t* base;   // start of the 160-byte fixed part
	const uint8_t* world;  // world-space vertices, 16 bytes each
};

VKR_DEV light_ref get_light(const shade_params& p, uint32_t index) {
	uint32_t vmax = p.max_light_vertex_count;
	uint32_t stride = 160 + 16 * vmax * 2 + 16 * (vmax - 2);
	light_ref l;
	l.base = p.constants + 256 + stride * index;
	l.world = l.base + 160 + 16 * vmax;
	return l;
}
VKR_DEV f3 light_vertex(const light_ref& l, uint32_t i) { return load_f3(l.world, 16 * i); }
VKR_DEV uint32_t light_vertex_count(const light_ref& l) { return load_u(l.base, 80); }
VKR_DEV f3 light_radiance(const light_ref& l) { return load_f3(l.base, 48); }
VKR_DEV float plane_distance(const light_ref& l, f3 p) {
	return ((p.x * load_f(l.base, 64) + p.y * load_f(l.base, 68)) + p.z * load_f(l.base, 72)) + 1.0f * load_f(l.base, 76);
}
VKR_DEV f3 plane_normal(const light_ref& l) { return load_f3(l.base, 64); }
VKR_DEV f3 light_translation(const light_ref& l) { return load_f3(l.base, 16); }
// column k of the plane-to-world rotation (the uniform block is row_major)
VKR_DEV f3 light_rotation_column(const light_ref& l, uint32_t k) { return mk3(load_f(l.base, 96 + 4 * k), load_f(l.base, 112 + 4 * k), load_f(l.base, 128 + 4 * k)); }
VKR_DEV float light_area(const light_ref& l) { return load_f(l.base, 144); }
// (area of fan triangle i, area of the fan up to triangle i); the last entry holds the total
VKR_DEV f2 light_fan_area(const light_ref& l, uint32_t vmax, uint32_t i) { return mk2(load_f(l.world, 16 * vmax + 16 * i), load_f(l.world, 16 * vmax + 16 * i + 4)); }

// polygonal_light_ray_intersection, polygonal_light_utility.glsl:93-112
VKR_DEV bool light_ray_intersection(const light_ref& light, uint32_t vmax, f3 origin, f3 end_xyz, float end_w) {
	float side_a = plane_distance(light, origin);
	f3 n = plane_normal(light);
	float side_b = ((n.x * end_xyz.x + n.y * end_xyz.y) + n.z * end_xyz.z) + load_f(light.base, 76) * end_w;
	if (side_a * side_b > 0.0f) return false;
	f3 dir = end_xyz - origin * end_w;
	float previous_sign = 0.0f;
	bool result = true;
	uint32_t count = light_vertex_count(light);
	for (uint32_t i = 0; i != vmax; ++i) {
		f3 a = light_vertex(light, i) - origin;
		f3 b = light_vertex(light, (i + 1) % vmax) - origin;
		float sign = dir.x * (a.y * b.z - b.y * a.z) - a.x * (dir.y * b.z - b.y * dir.z) + b.x * (dir.y * a.z - a.y * dir.z);
		result = result && ((i >= 3 && i >= count) || previous_sign * sign >= 0.0f);
		previous_sign = sign;
	}
	return result;
}

// textureLod(g_light_textures[i], uv, 0.0f) with the sampler of reference main.c:611-621 (linear,
// u repeats, v clamps); same arithmetic as oracle_sample_light_texture
VKR_DEV f3 sample_light_texture(const shade_params& p, uint32_t texture_index, f2 uv) {
	uint4 d = p.light_texture_descriptors[texture_index];
	if (d.y == 0) return mk3(1.0f, 1.0f, 1.0f);
	float u = uv.x - floorf(uv.x), v = uv.y;
	if (!(u >= 0.0f && u <= 1.0f)) u = 0.0f;
	v = (v > 0.0f) ? ((v < 1.0f) ? v : 1.0f) : 0.0f;
	int w = (int) d.y, h = (int) d.z;
	float fx = u * (float) w - 0.5f, fy = v * (float) h - 0.5f;
	float flx = floorf(fx), fly = floorf(fy);
	float wx = fx - flx, wy = fy - fly;
	int ix = (int) flx, iy = (int) fly;
	int x0 = (ix < 0) ? w - 1 : ix, x1 = (ix + 1 >= w) ? 0 : ix + 1;
	int y0 = (iy < 0) ? 0 : iy, y1 = (iy + 1 >= h) ? h - 1 : iy + 1;
	const float4* texels = p.light_texels + d.x;
	float4 t00 = texels[(size_t) y0 * w + x0], t10 = texels[(size_t) y0 * w + x1];
	float4 t01 = texels[(size_t) y1 * w + x0], t11 = texels[(size_t) y1 * w + x1];
	float one_minus_wx = 1.0f - wx, one_minus_wy = 1.0f - wy;
	f3 top = mk3(t00.x * one_minus_wx + t10.x * wx, t00.y * one_minus_wx + t10.y * wx, t00.z * one_minus_wx + t10.z * wx);
	f3 bottom = mk3(t01.x * one_minus_wx + t11.x * wx, t01.y * one_minus_wx + t11.y * wx, t01.z * one_minus_wx + t11.z * wx);
	return mk3(top.x * one_minus_wy + bottom.x * wy, top.y * one_minus_wy + bottom.y * wy, top.z * one_minus_wy + bottom.z * wy);
}

// get_polygon_radiance, shading_pass.frag.glsl:151-185.  TEXTURED is a property of the kernel
// variant (the host picks it when any light has a texturing technique): the extra live registers
// would otherwise cost the untextured variants a wave of occupancy.
template <bool TEXTURED>
VKR_DEV f3 polygon_radiance(const shade_params& p, f3 dir, f3 position, const light_ref& light) {
	f3 radiance = light_radiance(light);
	if constexpr (!TEXTURED) return radiance;
	uint32_t technique = load_u(light.base, 84);
	if (technique != 0 && p.light_texture_descriptors) {
		f2 uv;
		if (technique == 1) {
			// polygon_texturing_area: plane-space coordinates of the point that the ray hits
			float t = divide(-plane_distance(light, position), dot(dir, plane_normal(light)));
			f3 x = (position + dir * t) - light_translation(light);
			uv.x = dot(light_rotation_column(light, 0), x) * load_f(light.base, 44);
			uv.y = dot(light_rotation_column(light, 1), x) * load_f(light.base, 60);
		}
		else {
			f3 lookup;
			if (technique == 3) {
				// polygon_texturing_ies_profile: plane space; the profile contains the cosine
				lookup = mk3(dot(light_rotation_column(light, 0), dir), dot(light_rotation_column(light, 1), dir), dot(light_rotation_column(light, 2), dir));
				radiance = radiance * divide(1.0f, fabsf(lookup.z));
			}
			else
				// polygon_texturing_portal: light probe parametrisation
				lookup = mk3(-dir.x, dir.y, dir.z);
			uv.x = arctan2(lookup.y, lookup.x) * (0.5f * kInvPi);
			uv.y = arccos(lookup.z) * kInvPi;
		}
		radiance = radiance * sample_light_texture(p, load_u(light.base, 88), uv);
	}
	return radiance;
}

}  // namespace vkr
