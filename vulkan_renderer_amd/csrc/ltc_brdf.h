// The linearly transformed cosine of a shading point and the BRDF: Frostbite diffuse, GGX specular, and the GGX
// sampling of the visible normals.
//
// Follows reference src/shaders/ltc_utility.glsl:58-108 and src/shaders/brdfs.glsl.
#pragma once
#include "shading_inputs.h"

namespace vkr {

// ---- LTC (ltc_utility.glsl:58-108) ---------------------------------------------------

struct ltc_coefficients {
	m43 world_to_shading;
	m43 world_to_cosine;
	// shading_to_cosine = [[m00, 0, m02], [0, m11, 0], [m20, 0, m22]] (row, column)
	float m00, m02, m11, m20, m22;
	// cosine_to_shading, same sparsity
	float i00, i02, i11, i20, i22;
	float albedo, determinant;
};

VKR_DEV f3 shading_to_cosine(const ltc_coefficients& l, f3 v) {
	// column-major product with the structural zeros kept (they matter for -0)
	return mk3((l.m00 * v.x + 0.0f * v.y) + l.m02 * v.z, (0.0f * v.x + l.m11 * v.y) + 0.0f * v.z, (l.m20 * v.x + 0.0f * v.y) + l.m22 * v.z);
}
VKR_DEV f3 cosine_to_shading(const ltc_coefficients& l, f3 v) {
	return mk3((l.i00 * v.x + 0.0f * v.y) + l.i02 * v.z, (0.0f * v.x + l.i11 * v.y) + 0.0f * v.z, (l.i20 * v.x + 0.0f * v.y) + l.i22 * v.z);
}

VKR_DEV float bilinear(float t00, float t10, float t01, float t11, float wx, float wy) {
	float top = t00 * (1.0f - wx) + t10 * wx;
	float bottom = t01 * (1.0f - wx) + t11 * wx;
	return top * (1.0f - wy) + bottom * wy;
}

VKR_DEV ltc_coefficients get_ltc_coefficients(const shade_params& p, float fresnel_0, float roughness, f3 position, f3 normal, f3 outgoing) {
	const uint8_t* c = p.constants;
	ltc_coefficients l;
	float n_dot_o = dot(normal, outgoing);
	float inclination = arccos_unit(gclamp(n_dot_o, 0.0f, 1.0f));
	float u = fmaf(square_root(gclamp(roughness, 0.0f, 1.0f)), load_f(c, 232), load_f(c, 236));
	float v = fmaf(inclination, load_f(c, 240), load_f(c, 244));
	float w = fmaf(gclamp(fresnel_0, 0.0f, 1.0f), load_f(c, 224), load_f(c, 228));
	// bilinear, clamp to edge, nearest layer; exact fp32 weights, x first
	int res = (int) p.ltc_resolution;
	float fx = u * (float) res - 0.5f, fy = v * (float) res - 0.5f;
	float flx = floorf(fx), fly = floorf(fy);
	float wx = fx - flx, wy = fy - fly;
	int x0 = (int) flx, y0 = (int) fly;
	int x1 = min(max(x0 + 1, 0), res - 1), y1 = min(max(y0 + 1, 0), res - 1);
	x0 = min(max(x0, 0), res - 1);
	y0 = min(max(y0, 0), res - 1);
	int layer = min(max((int) rintf(w), 0), (int) p.ltc_layer_count - 1);
	size_t base = (size_t) layer * res * res;
	size_t i00 = base + (size_t) y0 * res + x0, i10 = base + (size_t) y0 * res + x1;
	size_t i01 = base + (size_t) y1 * res + x0, i11 = base + (size_t) y1 * res + x1;
	uint2 a00 = p.ltc_rgba[i00], a10 = p.ltc_rgba[i10], a01 = p.ltc_rgba[i01], a11 = p.ltc_rgba[i11];
	uint32_t b00 = p.ltc_rg[i00], b10 = p.ltc_rg[i10], b01 = p.ltc_rg[i01], b11 = p.ltc_rg[i11];
	float d0 = bilinear(unorm16(a00.x & 0xFFFF), unorm16(a10.x & 0xFFFF), unorm16(a01.x & 0xFFFF), unorm16(a11.x & 0xFFFF), wx, wy);
	float d1 = bilinear(unorm16(a00.x >> 16), unorm16(a10.x >> 16), unorm16(a01.x >> 16), unorm16(a11.x >> 16), wx, wy);
	float d2 = bilinear(unorm16(a00.y & 0xFFFF), unorm16(a10.y & 0xFFFF), unorm16(a01.y & 0xFFFF), unorm16(a11.y & 0xFFFF), wx, wy);
	float d3 = bilinear(unorm16(a00.y >> 16), unorm16(a10.y >> 16), unorm16(a01.y >> 16), unorm16(a11.y >> 16), wx, wy);
	float d4 = bilinear(unorm16(b00 & 0xFFFF), unorm16(b10 & 0xFFFF), unorm16(b01 & 0xFFFF), unorm16(b11 & 0xFFFF), wx, wy);
	float d5 = bilinear(unorm16(b00 >> 16), unorm16(b10 >> 16), unorm16(b01 >> 16), unorm16(b11 >> 16), wx, wy);
	// mat3(d0, 0, -d1,  0, d2, 0,  d3, 0, d4) column by column
	l.m00 = d0; l.m20 = -d1; l.m11 = d2; l.m02 = d3; l.m22 = d4;
	l.albedo = d5;
	float det2 = d0 * d4 + d1 * d3;
	l.determinant = d2 * det2;
	float inv_det2 = rcp(det2);
	l.i00 = d4 * inv_det2; l.i20 = d1 * inv_det2; l.i11 = rcp(d2); l.i02 = -d3 * inv_det2; l.i22 = d0 * inv_det2;
	f3 x_axis = normalize(fma3(-n_dot_o, normal, outgoing));
	f3 y_axis = cross(normal, x_axis);
	f3 r0 = mk3(x_axis.x, y_axis.x, normal.x);
	f3 r1 = mk3(x_axis.y, y_axis.y, normal.y);
	f3 r2 = mk3(x_axis.z, y_axis.z, normal.z);
	l.world_to_shading.c[0] = r0;
	l.world_to_shading.c[1] = r1;
	l.world_to_shading.c[2] = r2;
	m3 neg;
	neg.c[0] = -r0; neg.c[1] = -r1; neg.c[2] = -r2;
	l.world_to_shading.c[3] = mul(neg, position);
#pragma unroll
	for (int i = 0; i < 4; ++i) l.world_to_cosine.c[i] = shading_to_cosine(l, l.world_to_shading.c[i]);
	return l;
}

VKR_DEV float evaluate_ltc_density(const ltc_coefficients& l, f3 dir_shading, float rcp_psa) {
	f3 dc = shading_to_cosine(l, dir_shading);
	float len_sq = dot(dc, dc);
	float density = divide(gmax(0.0f, dc.z) * l.determinant, len_sq * len_sq);
	return density * rcp_psa;
}

// ---- BRDF (brdfs.glsl) -------------------------------------------------------------

VKR_DEV float schlick(float f0, float f90, float cos_theta) {
	float flipped = 1.0f - cos_theta;
	float flipped_squared = flipped * flipped;
	return f0 + (f90 - f0) * (flipped_squared * flipped * flipped_squared);
}

template <bool DIFFUSE, bool SPECULAR>
VKR_DEV f3 evaluate_brdf(const shading_data& d, f3 incoming) {
	f3 half_sum = incoming + d.outgoing;
	f3 half_vector = half_sum * rsqrt(dot(half_sum, half_sum));
	float lambert_incoming = dot(d.normal, incoming);
	float outgoing_dot_half = dot(d.outgoing, half_vector);
	f3 brdf = mk3(0.0f, 0.0f, 0.0f);
	if (DIFFUSE) {
		float f90 = fmaf(outgoing_dot_half * outgoing_dot_half, 2.0f * d.roughness, 0.5f);
		float product = schlick(1.0f, f90, d.lambert_outgoing) * schlick(1.0f, f90, lambert_incoming);
		brdf = brdf + d.diffuse_albedo * product;
	}
	if (SPECULAR) {
		float normal_dot_half = dot(d.normal, half_vector);
		float a2 = d.roughness * d.roughness;
		float ggx = fmaf(fmaf(normal_dot_half, a2, -normal_dot_half), normal_dot_half, 1.0f);
		ggx = divide(a2, ggx * ggx);
		float masking = lambert_incoming * square_root(fmaf(fmaf(-d.lambert_outgoing, a2, d.lambert_outgoing), d.lambert_outgoing, a2));
		float shadowing = d.lambert_outgoing * square_root(fmaf(fmaf(-lambert_incoming, a2, lambert_incoming), lambert_incoming, a2));
		float smith = divide(0.5f, masking + shadowing);
		float ct = gclamp(outgoing_dot_half, 0.0f, 1.0f);
		float gs = ggx * smith;
		brdf = brdf + mk3(gs * schlick(d.fresnel_0.x, 1.0f, ct), gs * schlick(d.fresnel_0.y, 1.0f, ct), gs * schlick(d.fresnel_0.z, 1.0f, ct));
	}
	return brdf * kInvPi;
}

VKR_DEV float ggx_vndf_density(float out_dot_n, float micro_dot_n, float micro_dot_out, float roughness) {
	float a2 = roughness * roughness;
	float ggx = fmaf(fmaf(micro_dot_n, a2, -micro_dot_n), micro_dot_n, 1.0f);
	ggx = divide(a2, ggx * ggx);
	ggx *= kInvPi;
	float masking = square_root(fmaf(fmaf(-out_dot_n, a2, out_dot_n), out_dot_n, a2));
	masking = divide(2.0f, out_dot_n + masking);
	return masking * micro_dot_out * ggx;
}

VKR_DEV f3 sample_ggx_vndf(f3 out_shading, float rx, float ry, f2 u) {
	m3 e2h;
	e2h.c[2] = normalize(mk3(rx * out_shading.x, ry * out_shading.y, 1.0f * out_shading.z));
	float length_sq = e2h.c[2].x * e2h.c[2].x + e2h.c[2].y * e2h.c[2].y;
	float inv_len = rsqrt(length_sq);
	e2h.c[0] = mk3(-e2h.c[2].y * inv_len, e2h.c[2].x * inv_len, 0.0f * inv_len);
	if (length_sq <= 0.0f) e2h.c[0] = mk3(1.0f, 0.0f, 0.0f);
	e2h.c[1] = cross(e2h.c[2], e2h.c[0]);
	float radius = square_root(u.x);
	float azimuth = (2.0f * kPi) * u.y;
	float sn, cs;
	sincos_poly(azimuth, sn, cs);
	f2 disk = mk2(radius * cs, radius * sn);
	f3 s;
	s.x = disk.x;
	float lerp = fmaf(0.5f, e2h.c[2].z, 0.5f);
	float a = square_root(fmaf(-disk.x, disk.x, 1.0f));
	s.y = a * (1.0f - lerp) + disk.y * lerp;
	s.z = square_root(gmax(0.0f, 1.0f - (s.x * s.x + s.y * s.y)));
	f3 hemi = mul(e2h, s);
	return normalize(mk3(rx * hemi.x, ry * hemi.y, 1.0f * hemi.z));
}

VKR_DEV f3 sample_ggx_reflected(float& out_density, f3 out_shading, float roughness, f2 u) {
	f3 micro = sample_ggx_vndf(out_shading, roughness, roughness, u);
	float micro_dot_out = dot(micro, out_shading);
	float density = ggx_vndf_density(out_shading.z, micro.z, micro_dot_out, roughness);
	f3 incoming = fma3(2.0f * micro_dot_out, micro, -out_shading);
	out_density = divide(density, 4.0f * micro_dot_out);
	return incoming;
}

VKR_DEV float ggx_reflected_density(float out_dot_n, f3 out_dir, f3 in_dir, f3 normal, float roughness) {
	f3 micro = normalize(out_dir + in_dir);
	float micro_dot_out = dot(micro, out_dir);
	float micro_dot_n = dot(micro, normal);
	float density = ggx_vndf_density(out_dot_n, micro_dot_n, micro_dot_out, roughness);
	return divide(density, 4.0f * micro_dot_out);
}

}  // namespace vkr
