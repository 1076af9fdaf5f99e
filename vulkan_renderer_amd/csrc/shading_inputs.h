// What a pixel's shading starts from: the loads of the frame constants, the noise accessor, the reconstruction of the
// shading point from the G-buffer with the material texture sampler, and where the pixel of a thread lies and its colour
// goes.  Shared by the shading kernels (shading_kernel.h), the resolve kernel (wavefront_kernels.h) and the shaft walk
// (light_shafts.h).
//
// Follows reference src/shaders/noise_utility.glsl:63-103 and src/shaders/shading_pass.frag.glsl (get_shading_data
// :721-822, the NaN guard and the exposure of main :861-866); the texture sampler is the oracle's
// (oracle_sample_texture in oracle/oracle_shading.c).
#pragma once
#include "shade_params.h"
#include "device_math.h"

namespace vkr {

// Reads of the constant buffer (frame constants and light records; written by the host before the
// launch, never by a kernel) go through the constant address space: the compiler may then use scalar
// loads for the wave-uniform addresses and keep or re-load the values as it likes.  As plain global
// loads they became vector loads with a full s_waitcnt inside the sampling loops - after the first
// store of a term nothing proves to the compiler that the buffer is still what it was.
typedef const __attribute__((address_space(4))) float* constant_float_pointer;
typedef const __attribute__((address_space(4))) uint32_t* constant_uint_pointer;
VKR_DEV float load_f(const uint8_t* base, uint32_t offset) { return *(constant_float_pointer) (uintptr_t) (base + offset); }
VKR_DEV uint32_t load_u(const uint8_t* base, uint32_t offset) { return *(constant_uint_pointer) (uintptr_t) (base + offset); }
VKR_DEV f3 load_f3(const uint8_t* base, uint32_t offset) { return mk3(load_f(base, offset), load_f(base, offset + 4), load_f(base, offset + 8)); }

VKR_DEV float unorm16(uint32_t v) {
#if VKR_FAST_MATH
	return (float) v * (1.0f / 65535.0f);
#else
	return divide((float) v, 65535.0f);
#endif
}

// ---- noise (noise_utility.glsl:63-103) ---------------------------------------------

// The texel of the NEXT fetch is requested as soon as the current one has been unpacked :
// a fetch is the one vector load of a sample, and it used to be waited for right where it was issued -
// which, on this hardware, also means waiting for every store before it: loads and stores share the
// vector-memory counter and complete out of order with each other, so the wait for a load with stores in
// flight is a wait for all of them (s_waitcnt vmcnt(0): the terms and rays of the sample before, a round
// trip to the L2).  With the request a sample ahead and the wait pinned in front of the sample's own stores
// (settle_noise(), called by accumulate()) both the load and the earlier stores have long completed
// when the wave asks.  Two more live registers.
struct noise_accessor {
	float n0, n1, n2, n3;
	uint32_t available, px, py, sample_index;
	uint32_t ahead_x, ahead_y;  // texel of fetch number sample_index, on its way or there
};

VKR_DEV uint2 fetch_noise_texel(const shade_params& p, const noise_accessor& a) {
	const uint8_t* c = p.constants;
	uint32_t s = a.sample_index;
	uint32_t r0 = load_u(c, 208), r1 = load_u(c, 212), r2 = load_u(c, 216), r3 = load_u(c, 220);
	if (s & 2) { uint32_t t0 = r0, t1 = r1; r0 = r2; r1 = r3; r2 = t0; r3 = t1; }
	if (s & 1) { r0 = r1; r1 = r2; r2 = r3; }
	uint32_t shift = (s & 124) >> 2;
	uint32_t layer = (r2 + s) & load_u(c, 192);
	uint32_t sx = (a.px + (r0 >> shift)) & load_u(c, 184);
	uint32_t sy = (a.py + (r1 >> shift)) & load_u(c, 188);
	return p.noise[((size_t) layer * p.noise_height + sy) * p.noise_width + sx];
}

VKR_DEV noise_accessor make_noise_accessor(const shade_params& p, uint32_t px, uint32_t py) {
	noise_accessor a;
	a.n0 = a.n1 = a.n2 = a.n3 = 0.0f;
	a.available = 0; a.px = px; a.py = py; a.sample_index = 0;
	a.ahead_x = a.ahead_y = 0u;
	uint2 texel = fetch_noise_texel(p, a);
	a.ahead_x = texel.x; a.ahead_y = texel.y;
	return a;
}

// The requested texel has to have arrived from here on (an empty statement that "uses" its registers)
VKR_DEV void settle_noise(noise_accessor& a) {
	asm volatile("" : "+v"(a.ahead_x), "+v"(a.ahead_y));
}

VKR_DEV f2 next_noise_2(const shade_params& p, noise_accessor& a) {
	if (a.available <= 1) {
		uint2 texel = make_uint2(a.ahead_x, a.ahead_y);
		a.n0 = unorm16(texel.x & 0xFFFF); a.n1 = unorm16(texel.x >> 16);
		a.n2 = unorm16(texel.y & 0xFFFF); a.n3 = unorm16(texel.y >> 16);
		a.available = 4;
		++a.sample_index;
		// (one texel beyond the last one a pixel uses: the coordinates wrap, the read is harmless)
		uint2 ahead = fetch_noise_texel(p, a);
		a.ahead_x = ahead.x; a.ahead_y = ahead.y;
	}
	a.available -= 2;
	f2 r = mk2(a.n0, a.n1);
	a.n0 = a.n2; a.n1 = a.n3;
	return r;
}

// ---- G-buffer reconstruction (shading_pass.frag.glsl:721-822) ------------------------

struct shading_data {
	f3 position, normal, outgoing;
	float lambert_outgoing;
	f3 diffuse_albedo, fresnel_0;
	float roughness;
};

VKR_DEV f3 decode_position(uint2 q, f3 factor, f3 summand) {
	float px = (float) (q.x & 0x1FFFFF);
	float py = (float) (((q.x & 0xFFE00000u) >> 21) | ((q.y & 0x3FF) << 11));
	float pz = (float) ((q.y & 0x7FFFFC00u) >> 10);
	return mk3(fmaf(px, factor.x, summand.x), fmaf(py, factor.y, summand.y), fmaf(pz, factor.z, summand.z));
}

VKR_DEV f3 decode_normal(float ox, float oy) {
	const float factor = 2.0f * (65534.0f / 65535.0f);
	const float summand = -(32768.0f / 65535.0f) * factor;
	ox = fmaf(ox, factor, summand);
	oy = fmaf(oy, factor, summand);
	f3 n = mk3(ox, oy, 1.0f - fabsf(ox) - fabsf(oy));
	float sx = (ox >= 0.0f) ? 1.0f : -1.0f;
	float sy = (oy >= 0.0f) ? 1.0f : -1.0f;
	if (n.z < 0.0f) {
		float nx = (1.0f - fabsf(n.y)) * sx;
		float ny = (1.0f - fabsf(n.x)) * sy;
		n.x = nx; n.y = ny;
	}
	return normalize(n);
}

// the first half of get_shading_data (:723-752): vertex fetch and the barycentrics of the view ray
struct triangle_hit {
	f3 pos[3], nrm[3];
	f2 uv[3];
	f3 e0, e1, to0, ray_cross_e1, e0_cross_to0;
	float rcp_det, b0, b1, b2;
};

VKR_DEV triangle_hit intersect_primitive(const shade_params& p, uint32_t primitive, f3 ray_direction) {
	const uint8_t* c = p.constants;
	f3 factor = load_f3(c, 0), summand = load_f3(c, 16), camera = load_f3(c, 144);
	triangle_hit t;
#pragma unroll
	for (int i = 0; i < 3; ++i) {
		size_t vi = (size_t) primitive * 3 + i;
		t.pos[i] = decode_position(p.positions[vi], factor, summand);
		uint2 q = p.normals_and_tex_coords[vi];
		t.nrm[i] = decode_normal(unorm16(q.x & 0xFFFF), unorm16(q.x >> 16));
		t.uv[i] = mk2(fmaf(unorm16(q.y & 0xFFFF), 8.0f, 0.0f), fmaf(unorm16(q.y >> 16), -8.0f, 1.0f));
	}
	t.e0 = t.pos[1] - t.pos[0]; t.e1 = t.pos[2] - t.pos[0];
	t.ray_cross_e1 = cross(ray_direction, t.e1);
	t.rcp_det = rcp(dot(t.e0, t.ray_cross_e1));
	t.to0 = camera - t.pos[0];
	t.b1 = t.rcp_det * dot(t.to0, t.ray_cross_e1);
	t.e0_cross_to0 = cross(t.e0, t.to0);
	t.b2 = -t.rcp_det * dot(ray_direction, t.e0_cross_to0);
	t.b0 = 1.0f - (t.b1 + t.b2);
	return t;
}

// ---- material textures: the software sampler (oracle_sample_texture in oracle/oracle_shading.c) ----

struct texture_view {
	const uint32_t* texels;  // RGBA8, all mip levels, finest first
	uint32_t width, height, mip_count;
	bool srgb;
};

VKR_DEV float4 fetch_texel(const shade_params& p, const texture_view& t, const uint32_t* level, int width, int height, int x, int y) {
	x = ((x % width) + width) % width;
	y = ((y % height) + height) % height;
	uint32_t texel = level[(size_t) y * (size_t) width + (size_t) x];
	uint32_t r = texel & 255u, g = (texel >> 8) & 255u, b = (texel >> 16) & 255u, a = texel >> 24;
	float4 out;
	out.x = t.srgb ? p.srgb_table[r] : (float) r * (1.0f / 255.0f);
	out.y = t.srgb ? p.srgb_table[g] : (float) g * (1.0f / 255.0f);
	out.z = t.srgb ? p.srgb_table[b] : (float) b * (1.0f / 255.0f);
	out.w = (float) a * (1.0f / 255.0f);
	return out;
}

// The texel that the floored coordinate x0 addresses, before the repeat: x0 itself wherever an int holds it, texel 0 at or
// beyond +-2^31 and for a NaN (texel_index() of oracle/oracle_shading.c; the conversion instruction alone would saturate and
// turn a NaN into 0, where the oracle's host returns INT_MIN)
VKR_DEV int texel_index(float x0) {
	return (x0 >= -2147483648.0f && x0 < 2147483648.0f) ? (int) x0 : 0;
}

VKR_DEV float4 sample_level(const shade_params& p, const texture_view& t, uint32_t level, float u, float v) {
	const uint32_t* texels = t.texels;
	int width = (int) t.width, height = (int) t.height;
	for (uint32_t l = 0; l != level; ++l) {
		texels += (size_t) width * (size_t) height;
		width = width > 1 ? width / 2 : 1;
		height = height > 1 ? height / 2 : 1;
	}
	float x = u * (float) width - 0.5f, y = v * (float) height - 0.5f;
	float x0 = floorf(x), y0 = floorf(y);
	float fx = x - x0, fy = y - y0;
	int ix = texel_index(x0), iy = texel_index(y0);
	float4 t00 = fetch_texel(p, t, texels, width, height, ix, iy);
	float4 t10 = fetch_texel(p, t, texels, width, height, ix + 1, iy);
	float4 t01 = fetch_texel(p, t, texels, width, height, ix, iy + 1);
	float4 t11 = fetch_texel(p, t, texels, width, height, ix + 1, iy + 1);
	float4 out;
	out.x = (t00.x * (1.0f - fx) + t10.x * fx) * (1.0f - fy) + (t01.x * (1.0f - fx) + t11.x * fx) * fy;
	out.y = (t00.y * (1.0f - fx) + t10.y * fx) * (1.0f - fy) + (t01.y * (1.0f - fx) + t11.y * fx) * fy;
	out.z = (t00.z * (1.0f - fx) + t10.z * fx) * (1.0f - fy) + (t01.z * (1.0f - fx) + t11.z * fx) * fy;
	out.w = (t00.w * (1.0f - fx) + t10.w * fx) * (1.0f - fy) + (t01.w * (1.0f - fx) + t11.w * fx) * fy;
	return out;
}

// textureGrad with the sampler of src/scene.c:546-552 (linear filters, repeat addressing, 16x anisotropy), operation for
// operation oracle_sample_texture() of oracle/oracle_shading.c: what the Vulkan specification sketches as anisotropic
// filtering - N = min(ceil(P_max / P_min), 16, ceil(P_max)) trilinear taps at level log2(P_max / N), spread along the longer
// axis of the footprint at uv + (i / (N + 1) - 1 / 2) d(uv) and averaged in order; N = 1 is the isotropic trilinear sample of
// rounds 1 - 4 in every bit.  (The quotients may have any operands - a derivative of zero, a footprint of a thousand texels:
// the full-range division.)
// Every input has a defined result, the same on the host and on the device: a texel coordinate floor(u * width - 1 / 2) that
// no int holds - at or beyond +-2^31, NaN - addresses texel 0 of its axis (texel_index()).  Such a float has no fractional
// part, so a large finite coordinate returns that texel alone; an infinite or NaN coordinate gives a NaN sample.
constexpr float kMaxAnisotropy = 16.0f;
VKR_DEV float4 sample_texture(const shade_params& p, const texture_view& t, f2 uv, f2 duv_dx, f2 duv_dy) {
	float w = (float) t.width, h = (float) t.height;
	float ax = duv_dx.x * w, ay = duv_dx.y * h, bx = duv_dy.x * w, by = duv_dy.y * h;
	float px = square_root(ax * ax + ay * ay), py = square_root(bx * bx + by * by);
	bool x_major = px >= py;
	float p_max = gmax(px, py), p_min = x_major ? py : px;
	float taps = ceilf(divide_full_range(p_max, p_min));
	taps = gmin(gmin(taps, kMaxAnisotropy), gmax(ceilf(p_max), 1.0f));
	if (!(taps >= 1.0f)) taps = 1.0f;
	float rho = divide_full_range(p_max, taps);
	float max_level = (float) (t.mip_count - 1);
	float lambda = (rho > 1.0f) ? gmin(log2_poly(rho), max_level) : 0.0f;
	float level_0 = floorf(lambda);
	float fraction = lambda - level_0;
	uint32_t l0 = (uint32_t) level_0;
	uint32_t l1 = (l0 + 1 < t.mip_count) ? l0 + 1 : l0;
	uint32_t count = (uint32_t) taps;
	float du = x_major ? duv_dx.x : duv_dy.x, dv = x_major ? duv_dx.y : duv_dy.y;
	float4 sum = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	for (uint32_t i = 0; i != count; ++i) {
		float u = uv.x, v = uv.y;
		if (count > 1) {
			float offset = divide_full_range((float) (i + 1), taps + 1.0f) - 0.5f;
			u = u + du * offset;
			v = v + dv * offset;
		}
		float4 c0 = sample_level(p, t, l0, u, v), c1 = sample_level(p, t, l1, u, v);
		float4 tap = make_float4(c0.x * (1.0f - fraction) + c1.x * fraction, c0.y * (1.0f - fraction) + c1.y * fraction,
			c0.z * (1.0f - fraction) + c1.z * fraction, c0.w * (1.0f - fraction) + c1.w * fraction);
		sum = (count > 1) ? make_float4(sum.x + tap.x, sum.y + tap.y, sum.z + tap.z, sum.w + tap.w) : tap;
	}
	if (count > 1) sum = make_float4(divide_full_range(sum.x, taps), divide_full_range(sum.y, taps), divide_full_range(sum.z, taps), divide_full_range(sum.w, taps));
	return sum;
}

// The texture reads of get_shading_data (:754-785) for one pixel: screen-space derivatives of the
// barycentrics and of the texture coordinate, then base colour, specular and normal texture.
// Writes the eight numbers that a constant material stores (see materials_t.host_constants).
VKR_DEV void resolve_material(const shade_params& p, uint32_t primitive, f3 ray_direction, float (&out)[8]) {
	triangle_hit t = intersect_primitive(p, primitive, ray_direction);
	const uint8_t* c = p.constants;
	f3 derivs[2];
#pragma unroll
	for (int i = 0; i < 2; ++i) {
		f3 ray_deriv = mk3(load_f(c, 96 + 4 * i), load_f(c, 112 + 4 * i), load_f(c, 128 + 4 * i));
		f3 ray_cross_e1_deriv = cross(ray_deriv, t.e1);
		float rcp_det_deriv = -dot(t.e0, ray_cross_e1_deriv) * t.rcp_det * t.rcp_det;
		float det_0_dir_e1 = dot(t.to0, t.ray_cross_e1);
		float det_0_dir_e1_deriv = dot(t.to0, ray_cross_e1_deriv);
		derivs[i].y = rcp_det_deriv * det_0_dir_e1 + t.rcp_det * det_0_dir_e1_deriv;
		float det_dir_e0_0 = dot(ray_direction, t.e0_cross_to0);
		float det_dir_e0_0_deriv = dot(ray_deriv, t.e0_cross_to0);
		derivs[i].z = -rcp_det_deriv * det_dir_e0_0 - t.rcp_det * det_dir_e0_0_deriv;
		derivs[i].x = -(derivs[i].y + derivs[i].z);
	}
	f2 tex_coord = fma2(t.b0, t.uv[0], fma2(t.b1, t.uv[1], t.uv[2] * t.b2));
	f2 tex_derivs[2];
#pragma unroll
	for (int i = 0; i < 2; ++i) {
		f2 sum = mk2(0.0f, 0.0f);
		sum = sum + t.uv[0] * derivs[i].x;
		sum = sum + t.uv[1] * derivs[i].y;
		sum = sum + t.uv[2] * derivs[i].z;
		tex_derivs[i] = sum;
	}
	uint32_t material = p.material_indices[primitive];
	const float* constants = p.material_constants + 8 * (size_t) material;
#pragma unroll
	for (int type = 0; type < 3; ++type) {
		const uint32_t* descriptor = p.texture_descriptors + 4 * (3 * (size_t) material + type);
		float4 texel = make_float4(constants[3 * type], constants[3 * type + 1], type < 2 ? constants[3 * type + 2] : 0.0f, 1.0f);
		if (descriptor[1] != 0) {
			texture_view view;
			view.texels = p.texels + descriptor[0];
			view.width = descriptor[1]; view.height = descriptor[2];
			view.mip_count = descriptor[3] & 0xFFFFu;
			view.srgb = (descriptor[3] >> 16) != 0;
			texel = sample_texture(p, view, tex_coord, tex_derivs[0], tex_derivs[1]);
		}
		out[3 * type] = texel.x;
		out[3 * type + 1] = texel.y;
		if (type < 2) out[3 * type + 2] = texel.z;
	}
}

VKR_DEV shading_data get_shading_data(const shade_params& p, uint32_t primitive, f3 ray_direction, size_t pixel_index) {
	const uint8_t* c = p.constants;
	f3 camera = load_f3(c, 144);
	shading_data r;
	triangle_hit t = intersect_primitive(p, primitive, ray_direction);
	const f3 (&pos)[3] = t.pos;
	const f3 (&nrm)[3] = t.nrm;
	const f2 (&uv)[3] = t.uv;
	f3 e0 = t.e0, e1 = t.e1;
	float b0 = t.b0, b1 = t.b1, b2 = t.b2;
	r.position = fma3(b0, pos[0], fma3(b1, pos[1], pos[2] * b2));
	f3 interpolated_normal = normalize(fma3(b0, nrm[0], fma3(b1, nrm[1], nrm[2] * b2)));
	// constant material, or what the material resolve kernel sampled for this pixel
	const float* mc = p.pixel_materials ? p.pixel_materials + 8 * pixel_index : p.material_constants + 8 * (size_t) p.material_indices[primitive];
	f3 base_color = mk3(mc[0], mc[1], mc[2]);
	float linear_roughness = mc[4], metalicity = mc[5];
	f3 nt;
	nt.x = fmaf(mc[6], 2.0f, -1.0f);
	nt.y = fmaf(mc[7], 2.0f, -1.0f);
	nt.z = square_root(gmax(0.0f, fmaf(-nt.x, nt.x, fmaf(-nt.y, nt.y, 1.0f))));
	r.diffuse_albedo = mk3(fmaf(base_color.x, -metalicity, base_color.x), fmaf(base_color.y, -metalicity, base_color.y), fmaf(base_color.z, -metalicity, base_color.z));
	float dielectric = 0.02f * (1.0f - metalicity);
	r.fresnel_0 = mk3(dielectric + base_color.x * metalicity, dielectric + base_color.y * metalicity, dielectric + base_color.z * metalicity);
	r.roughness = linear_roughness * linear_roughness;
	r.roughness = gclamp(r.roughness * load_f(c, 180), 0.0064f, 1.0f);
	f2 uv_e0 = uv[1] - uv[0], uv_e1 = uv[2] - uv[0];
	f3 n_cross_e0 = cross(interpolated_normal, e0);
	f3 e1_cross_n = cross(e1, interpolated_normal);
	f3 tangent = e1_cross_n * uv_e0.x + n_cross_e0 * uv_e1.x;
	f3 bitangent = e1_cross_n * uv_e0.y + n_cross_e0 * uv_e1.y;
	float mean_tangent_length = square_root(0.5f * (dot(tangent, tangent) + dot(bitangent, bitangent)));
	m3 t2w;
	t2w.c[0] = tangent; t2w.c[1] = bitangent; t2w.c[2] = interpolated_normal;
	nt.z *= gmax(1.0e-10f, mean_tangent_length);
	r.normal = normalize(mul(t2w, nt));
	r.outgoing = normalize(camera - r.position);
	float normal_offset = gmax(0.0f, 1.0e-3f - dot(r.normal, r.outgoing));
	r.normal = fma3(normal_offset, r.outgoing, r.normal);
	r.normal = normalize(r.normal);
	r.lambert_outgoing = dot(r.normal, r.outgoing);
	return r;
}

// ---- the pixel of a thread and its output ------------------------------------------------

// Maps a thread of the frame to a pixel and its output slot.  `block` counts the 16x16 pixel
// blocks of the tiles this rank owns, `thread` the 256 pixels of a block; a wave is an 8x8 patch.
// Thread number block * 256 + thread is what the per-thread wavefront buffers are indexed by.
VKR_DEV bool locate_pixel(const shade_params& p, uint32_t block, uint32_t thread, uint32_t& px, uint32_t& py, size_t& out_index) {
	uint32_t blocks_per_side = p.tile_size >> 4;
	uint32_t blocks_per_tile = blocks_per_side * blocks_per_side;
	uint32_t local_tile = block / blocks_per_tile;
	uint32_t block_in_tile = block - local_tile * blocks_per_tile;
	uint32_t tile = local_tile * p.rank_count + p.rank;
	if (tile >= p.tile_count) return false;
	uint32_t ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
	uint32_t by = block_in_tile / blocks_per_side, bx = block_in_tile - by * blocks_per_side;
	uint32_t wave = thread >> 6, lane = thread & 63;
	uint32_t ix = (bx << 4) + ((wave & 1) << 3) + (lane & 7);
	uint32_t iy = (by << 4) + ((wave >> 1) << 3) + (lane >> 3);
	px = tx * p.tile_size + ix;
	py = ty * p.tile_size + iy;
	if (!p.slab_layout) out_index = (size_t) py * p.width + px;
	else out_index = (size_t) local_tile * p.tile_size * p.tile_size + (size_t) iy * p.tile_size + ix;
	return px < p.width && py < p.height;
}

VKR_DEV void store_final_color(const shade_params& p, size_t out_index, f3 color) {
	float exposure = load_f(p.constants, 176);
	bool broken = !(fabsf(color.x) < __builtin_inff()) || !(fabsf(color.y) < __builtin_inff()) || !(fabsf(color.z) < __builtin_inff());
	if (broken) color = mk3(divide(1.0f, exposure), divide(0.0f, exposure), divide(0.8f, exposure));
	p.out_radiance[out_index] = make_float4(color.x * exposure, color.y * exposure, color.z * exposure, 1.0f);
}

}  // namespace vkr
