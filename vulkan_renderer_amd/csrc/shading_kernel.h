// The per-pixel shading program as a HIP kernel for gfx950 (CDNA4).
//
// One lane per pixel; a workgroup is one wave64 and covers an 8x8 pixel patch (the four patches
// of a 16x16 block run on the same XCD), so neighbouring lanes read neighbouring triangles,
// LTC texels and noise texels and mostly agree on the clipping / sector branches.
// All uniform inputs (frame constants, light records) are read through wave-uniform
// addresses in the constant address space and end up in SGPRs.
//
// Follows reference src/shaders/shading_pass.frag.glsl (main :824-866,
// evaluate_polygonal_light_shading :329-711, get_mis_estimate :270-323, error_to_color :80-114) with the
// variant axes of src/main.c:752-792 as template parameters (shade_params.h, the launch contract).  What the program
// is made of, each in a header of its own:
//   shading_inputs.h  constant loads, noise, get_shading_data, the pixel of a thread and its output
//   ltc_brdf.h        LTC coefficients, the BRDF, GGX sampling
//   light_records.h   the light records, their textures and radiance
//   shadow_terms.h    pixel_context, the ray queue, accumulate()
//   kept_polygons.h   prepared polygons and sector terms that are kept between launches
#pragma once
#include "polygon_sampling.h"
#include "related_work.h"
#include "lbvh.h"
#include "shade_params.h"
#include "shading_inputs.h"
#include "ltc_brdf.h"
#include "light_records.h"
#include "shadow_terms.h"
#include "kept_polygons.h"

namespace vkr {

// ---- MIS estimators (shading_pass.frag.glsl:270-323) -----------------------------------------

VKR_DEV float mis_weight_over_density(int heuristic, float sampled, float other) {
	if (heuristic == kMisBalance) return rcp(sampled + other);
	if (heuristic == kMisPower) return divide(sampled, sampled * sampled + other * other);
	return 0.0f;
}

VKR_DEV float mis_estimate_channel(int heuristic, float in, float s, float sd, float o, float od, float ve) {
	if (heuristic == kMisWeighted) {
		float weighted_sum = s * sd + o * od;
		return divide(s * in, weighted_sum);
	}
	if (heuristic == kMisOptimalClamped || heuristic == kMisOptimal) {
		float balance = rcp(sd + od);
		float weighted_sum = s * sd + o * od;
		if (heuristic == kMisOptimalClamped) {
			float weighted = divide(s, weighted_sum);
			float mixed = fmaf(-ve, balance, balance);
			mixed = fmaf(ve, weighted, mixed);
			return mixed * in;
		}
		return ve * s + balance * (in - ve * weighted_sum);
	}
	return mis_weight_over_density(heuristic, sd, od) * in;
}

VKR_DEV f3 mis_estimate(int heuristic, f3 integrand, f3 sw, float sd, f3 ow, float od, float ve) {
	return mk3(mis_estimate_channel(heuristic, integrand.x, sw.x, sd, ow.x, od, ve),
		mis_estimate_channel(heuristic, integrand.y, sw.y, sd, ow.y, od, ve),
		mis_estimate_channel(heuristic, integrand.z, sw.z, sd, ow.z, od, ve));
}

// get_mis_estimate (shading_pass.frag.glsl:270-293) for the two integrands a deferred term needs - its
// value if the shadow ray reaches the light and its value if not - in one go: everything that does not
// depend on the integrand (the balance weight 1 / (sd + od), per channel the weighted sum and its
// quotient) is evaluated once instead of once per integrand and channel.  The operations on each value
// are those of mis_estimate_channel, so the results are the same bits; what it saves is issue slots -
// per term 4 instead of 12 divisions with the clamped optimal heuristic of BASELINE configs 3 and 4.
VKR_DEV void mis_estimate_pair(int heuristic, f3 lit, f3 dark, f3 sw, float sd, f3 ow, float od, float ve, f3& out_lit, f3& out_dark) {
	const float s[3] = {sw.x, sw.y, sw.z}, o[3] = {ow.x, ow.y, ow.z};
	const float a[3] = {lit.x, lit.y, lit.z}, b[3] = {dark.x, dark.y, dark.z};
	float ra[3], rb[3];
	if (heuristic == kMisWeighted) {
#pragma unroll
		for (int c = 0; c != 3; ++c) {
			float weighted_sum = s[c] * sd + o[c] * od;
			ra[c] = divide(s[c] * a[c], weighted_sum);
			rb[c] = divide(s[c] * b[c], weighted_sum);
		}
	}
	else if (heuristic == kMisOptimalClamped || heuristic == kMisOptimal) {
		float balance = rcp(sd + od);
#pragma unroll
		for (int c = 0; c != 3; ++c) {
			float weighted_sum = s[c] * sd + o[c] * od;
			if (heuristic == kMisOptimalClamped) {
				float weighted = divide(s[c], weighted_sum);
				float mixed = fmaf(-ve, balance, balance);
				mixed = fmaf(ve, weighted, mixed);
				ra[c] = mixed * a[c];
				rb[c] = mixed * b[c];
			}
			else {
				ra[c] = ve * s[c] + balance * (a[c] - ve * weighted_sum);
				rb[c] = ve * s[c] + balance * (b[c] - ve * weighted_sum);
			}
		}
	}
	else {
		float weight = mis_weight_over_density(heuristic, sd, od);
#pragma unroll
		for (int c = 0; c != 3; ++c) {
			ra[c] = weight * a[c];
			rb[c] = weight * b[c];
		}
	}
	out_lit = mk3(ra[0], ra[1], ra[2]);
	out_dark = mk3(rb[0], rb[1], rb[2]);
}

// get_polygonal_light_mis_estimate, shading_pass.frag.glsl:305-323
template <int STRATEGY, int RAYS, bool TEXTURED>
VKR_DEV void add_light_mis_estimate(pixel_context& ctx, f3& result, f3 dir, float density, const shading_data& sd, const light_ref& light) {
	// (once per sample and on every path through it, so that no request is outstanding at the top of the loop)
	if (ctx.noise) settle_noise(*ctx.noise);
	float lambert;
	bool candidate;
	f3 rb = radiance_brdf<true, true, TEXTURED>(ctx.p, lambert, candidate, dir, sd, light);
	const f3 zero = mk3(0.0f, 0.0f, 0.0f);
	f3 visible_term = zero, hidden_term = zero;
	if (STRATEGY == kStrategyDiffuseOnly) {
		float factor = divide(lambert, density);
		visible_term = (density > 0.0f) ? rb * factor : zero;
		hidden_term = (density > 0.0f) ? zero * factor : zero;
	}
	else if (STRATEGY == kStrategyDiffuseGgxMis) {
		float ggx_density = ggx_reflected_density(sd.lambert_outgoing, sd.outgoing, dir, sd.normal, sd.roughness);
		float weight = mis_weight_over_density(ctx.p.mis_heuristic, density, ggx_density);
		visible_term = (rb * lambert) * weight;
		hidden_term = (zero * lambert) * weight;
	}
	accumulate<RAYS>(ctx, result, candidate, visible_term, hidden_term, dir, sd, light);
}

// ---- error display (shading_pass.frag.glsl:80-114, :489-494, :549-563) -------------------------

// error_to_color, shading_pass.frag.glsl:80-114: tab20b colours (linear Rec. 709), four
// shades per decade over five decades
__device__ const float k_tab20b[20][3] = {
	{0.04092f, 0.04374f, 0.19120f}, {0.08438f, 0.08866f, 0.36625f}, {0.14703f, 0.15593f, 0.62396f}, {0.33245f, 0.34191f, 0.73046f},
	{0.12477f, 0.19120f, 0.04092f}, {0.26225f, 0.36131f, 0.08438f}, {0.46208f, 0.62396f, 0.14703f}, {0.61721f, 0.70838f, 0.33245f},
	{0.26225f, 0.15293f, 0.03071f}, {0.50888f, 0.34191f, 0.04092f}, {0.79910f, 0.49102f, 0.08438f}, {0.79910f, 0.59720f, 0.29614f},
	{0.23074f, 0.04519f, 0.04092f}, {0.41789f, 0.06663f, 0.06848f}, {0.67244f, 0.11954f, 0.14703f}, {0.79910f, 0.30499f, 0.33245f},
	{0.19807f, 0.05286f, 0.17144f}, {0.37626f, 0.08228f, 0.29614f}, {0.61721f, 0.15293f, 0.50888f}, {0.73046f, 0.34191f, 0.67244f}};

VKR_DEV f3 error_to_color(const shade_params& p, float error) {
	float error_factor = load_f(p.constants, 28);
	error = gmin(gmax(fabsf(error_factor * error), 1.0f), p.error_max);
	// NaN (degenerate sample) is undefined in the reference (int(NaN)); defined as the first colour
	error = (error == error) ? error : 1.0f;
	float color_index = fmaf(log2_poly(error), p.error_scale, -0.0f);
	int index = (int) color_index;
	return mk3(k_tab20b[index][0], k_tab20b[index][1], k_tab20b[index][2]);
}

// the ERROR_DISPLAY_* branches, shading_pass.frag.glsl:489-494, :549-563
template <int V, bool BIASED>
VKR_DEV f3 display_sampling_error(const shade_params& p, const psa_polygon<V>& polygon, noise_accessor& noise) {
	f2 u = next_noise_2(p, noise);
	f3 dir = sample_psa<V, BIASED>(polygon, u);
	f3 e = psa_sampling_error<V>(polygon, u, dir);
	float error = (p.error_index == 0) ? e.x : ((p.error_index == 1) ? e.y : e.z);
	return divide3(error_to_color(p, error), load_f(p.constants, 176));
}

// ---- the shading of one light ------------------------------------------------------------------

// evaluate_polygonal_light_shading, shading_pass.frag.glsl:329-711
// PREPARED: kPreparedPlain, or one of the other two where prepared_polygons_apply() (shade_params.h)
template <int STRATEGY, int TECHNIQUE, int V, int RAYS, int ERROR = kErrorNone, int PREPARED = kPreparedPlain>
VKR_DEV f3 evaluate_light(pixel_context& ctx, const shading_data& sd, const ltc_coefficients& ltc_in, const light_ref& light, noise_accessor& noise) {
	const shade_params& p = ctx.p;
	constexpr bool kTextured = ERROR == kLightTextures;
	constexpr bool kBiased = TECHNIQUE == kTechniquePsaBiased;
	constexpr bool kIsPsa = TECHNIQUE == kTechniquePsa || TECHNIQUE == kTechniquePsaBiased;
	// (no request is outstanding when a sampling loop is entered - the first one was made when the pixel
	// started - or the wait for it would sit at the top of the loop and be paid by every sample)
	settle_noise(noise);
	const uint32_t S = p.sample_count;
	const uint32_t count = light_vertex_count(light);
	const f3 zero = mk3(0.0f, 0.0f, 0.0f);
	f3 result = zero;
	float density_factor = 0.0f;
	m43 world_to_shading = ltc_in.world_to_shading;

	if constexpr (TECHNIQUE == kTechniqueBaseline) {
		// shading_pass.frag.glsl:332-342: not a sampler, the run time baseline of the paper
		f3 corner_offset = light_translation(light) - sd.position;
		f3 r0 = light_rotation_column(light, 0), r1 = light_rotation_column(light, 1);
		for (uint32_t s = 0; s != S; ++s) {
			f2 u = next_noise_2(p, noise);
			f3 dir = normalize((corner_offset + r0 * u.x) + r1 * u.y);
			add_light_mis_estimate<STRATEGY, RAYS, kTextured>(ctx, result, dir, 1.0f, sd, light);
		}
	}
	else if constexpr (TECHNIQUE == kTechniqueAreaTurk) {
		// uniform area sampling (Turk), polygon_sampling_related_work.glsl:38-85
		const uint32_t vmax = p.max_light_vertex_count;
		for (uint32_t s = 0; s != S; ++s) {
			f2 u = next_noise_2(p, noise);
			float target_area = light_fan_area(light, vmax, vmax - 3).y * u.x;
			float subtriangle_area = target_area;
			float triangle_area = light_fan_area(light, vmax, 0).x;
			f3 t0 = light_vertex(light, 1), t1 = light_vertex(light, 0), t2 = light_vertex(light, 2);
			bool done = false;
			for (uint32_t i = 0; i + 3 < vmax; ++i) {
				f2 fan = light_fan_area(light, vmax, i);
				done = done || i + 3 >= count || fan.y >= target_area;
				if (!done) {
					subtriangle_area = target_area - fan.y;
					triangle_area = light_fan_area(light, vmax, i + 1).x;
					t0 = light_vertex(light, i + 2);
					t2 = light_vertex(light, i + 3);
				}
			}
			float sqrt_u = square_root(divide(subtriangle_area, triangle_area));
			float b0 = 1.0f - sqrt_u, b1 = sqrt_u * u.y, b2 = fmaf(-sqrt_u, u.y, sqrt_u);
			f3 light_sample = (t0 * b0 + t1 * b1) + t2 * b2;
			f3 d = light_sample - sd.position;
			float distance_squared = dot(d, d);
			f3 dir = d * rsqrt(distance_squared);
			float projected_area = fabsf(dot(plane_normal(light), dir)) * light_area(light);
			add_light_mis_estimate<STRATEGY, RAYS, kTextured>(ctx, result, dir, divide(distance_squared, projected_area), sd, light);
		}
	}
	else if constexpr (TECHNIQUE == kTechniqueUrena) {
		// shading_pass.frag.glsl:352-362: the light is taken to be the unit square of its plane
		urena_rectangle pd = prepare_urena(light_translation(light), load_f(light.base, 12), load_f(light.base, 28),
			light_rotation_column(light, 0), light_rotation_column(light, 1), light_rotation_column(light, 2), sd.position);
		density_factor = rcp(pd.solid_angle);
		for (uint32_t s = 0; s != S; ++s) {
			f3 dir = sample_urena(pd, next_noise_2(p, noise));
			add_light_mis_estimate<STRATEGY, RAYS, kTextured>(ctx, result, dir, density_factor, sd, light);
		}
	}
	else if constexpr (TECHNIQUE == kTechniqueArvoSolidAngle) {
		// :364-373
		f3 vw[V];
#pragma unroll
		for (int i = 0; i < V; ++i) vw[i] = light_vertex(light, min((uint32_t) i, p.max_light_vertex_count - 1));
		arvo_polygon<V> pd;
		prepare_arvo<V>(pd, count, vw, sd.position);
		density_factor = rcp(pd.solid_angle);
		for (uint32_t s = 0; s != S; ++s) {
			f3 dir = sample_arvo<V>(pd, next_noise_2(p, noise));
			add_light_mis_estimate<STRATEGY, RAYS, kTextured>(ctx, result, dir, density_factor, sd, light);
		}
	}
	else if constexpr (TECHNIQUE == kTechniqueHartBilinear || TECHNIQUE == kTechniqueHartBilinearClipping
		|| TECHNIQUE == kTechniqueHartBiquadratic || TECHNIQUE == kTechniqueHartBiquadraticClipping)
	{
		// :386-438; without clipping the polygon keeps MAX_POLYGONAL_LIGHT_VERTEX_COUNT slots
		constexpr bool kClipping = TECHNIQUE == kTechniqueHartBilinearClipping || TECHNIQUE == kTechniqueHartBiquadraticClipping;
		constexpr bool kBiquadratic = TECHNIQUE == kTechniqueHartBiquadratic || TECHNIQUE == kTechniqueHartBiquadraticClipping;
		constexpr int kLightSlots = kClipping ? V - 1 : V;
		f3 vs[V];
#pragma unroll
		for (int i = 0; i < kLightSlots; ++i) vs[i] = mul_point(world_to_shading, light_vertex(light, min((uint32_t) i, p.max_light_vertex_count - 1)));
		if constexpr (kClipping) vs[V - 1] = zero;
		uint32_t clipped = count;
		if constexpr (kClipping) {
			clipped = clip_polygon<V>(count, vs);
			if (clipped == 0) return zero;
		}
		if constexpr (kBiquadratic) {
			hart_biquadratic<V> pd;
			prepare_hart_biquadratic<V>(pd, clipped, vs);
			for (uint32_t s = 0; s != S; ++s) {
				float density;
				f3 dir = sample_hart_biquadratic<V>(density, pd, next_noise_2(p, noise));
				dir = mul_transposed(world_to_shading, dir);
				add_light_mis_estimate<STRATEGY, RAYS, kTextured>(ctx, result, dir, density, sd, light);
			}
		}
		else {
			hart_bilinear<V> pd;
			prepare_hart_bilinear<V>(pd, clipped, vs);
			for (uint32_t s = 0; s != S; ++s) {
				float density;
				f3 dir = sample_hart_bilinear<V>(density, pd, next_noise_2(p, noise));
				dir = mul_transposed(world_to_shading, dir);
				add_light_mis_estimate<STRATEGY, RAYS, kTextured>(ctx, result, dir, density, sd, light);
			}
		}
	}
	else if constexpr (TECHNIQUE == kTechniqueSolidAngle) {
		f3 vw[V];
#pragma unroll
		for (int i = 0; i < V; ++i) vw[i] = light_vertex(light, min((uint32_t) i, p.max_light_vertex_count - 1));
		sa_polygon<V> pd;
		prepare_sa<V>(pd, count, vw, sd.position);
		density_factor = rcp(pd.solid_angle);
		for (uint32_t s = 0; s != S; ++s) {
			f3 dir = sample_sa<V>(pd, next_noise_2(p, noise));
			add_light_mis_estimate<STRATEGY, RAYS, kTextured>(ctx, result, dir, density_factor, sd, light);
		}
	}
	else if constexpr (TECHNIQUE == kTechniqueClippedSolidAngle) {
		f3 vs[V];
#pragma unroll
		for (int i = 0; i < V - 1; ++i) vs[i] = mul_point(world_to_shading, light_vertex(light, min((uint32_t) i, p.max_light_vertex_count - 1)));
		vs[V - 1] = zero;
		uint32_t clipped = clip_polygon<V>(count, vs);
		if (clipped == 0) return zero;
		sa_polygon<V> pd;
		prepare_sa<V>(pd, clipped, vs, zero);
		density_factor = rcp(pd.solid_angle);
		for (uint32_t s = 0; s != S; ++s) {
			f3 dir = sample_sa<V>(pd, next_noise_2(p, noise));
			dir = mul_transposed(world_to_shading, dir);
			add_light_mis_estimate<STRATEGY, RAYS, kTextured>(ctx, result, dir, density_factor, sd, light);
		}
	}
	else {
		// projected solid angle sampling; flip the frame if the shading point is
		// behind the light so that the winding stays clockwise (:444-449)
		m43 world_to_cosine = ltc_in.world_to_cosine;
		float side = plane_distance(light, sd.position);
		if (side < 0.0f) {
#pragma unroll
			for (int i = 0; i < 4; ++i) {
				world_to_shading.c[i].y = -world_to_shading.c[i].y;
				world_to_cosine.c[i].y = -world_to_cosine.c[i].y;
			}
		}
		if constexpr (STRATEGY == kStrategyDiffuseOnly || STRATEGY == kStrategyDiffuseGgxMis) {
			f3 vs[V];
#pragma unroll
			for (int i = 0; i < V - 1; ++i) vs[i] = mul_point(world_to_shading, light_vertex(light, min((uint32_t) i, p.max_light_vertex_count - 1)));
			vs[V - 1] = zero;
			uint32_t clipped = clip_polygon<V>(count, vs);
			if (clipped == 0) return zero;
			if constexpr (TECHNIQUE == kTechniquePsaArvo) {
				// Arvo's sampler, three Newton iterations (:462-481); the GGX tail below uses its
				// density without the cosine, like the reference
				psa_arvo<V> pa;
				prepare_psa_arvo<V>(pa, clipped, vs);
				if (pa.total <= 0.0f) return zero;
				if constexpr (ERROR == kErrorDiffuse) {
					f2 u = next_noise_2(p, noise);
					f3 dir = sample_psa_arvo<V>(pa, u, 3u);
					f2 e = psa_sampling_error_arvo<V>(pa, u, dir);
					return divide3(error_to_color(p, (p.error_index == 0) ? e.x : e.y), load_f(p.constants, 176));
				}
				for (uint32_t s = 0; s != S; ++s) {
					f3 dir = sample_psa_arvo<V>(pa, next_noise_2(p, noise), 3u);
					float density = divide(dir.z, pa.total);
					dir = mul_transposed(world_to_shading, dir);
					add_light_mis_estimate<STRATEGY, RAYS, kTextured>(ctx, result, dir, density, sd, light);
				}
				density_factor = rcp(pa.total);
			}
			else {
				psa_polygon<V> pd;
				prepare_psa<V, kBiased>(pd, clipped, vs);
				if (pd.total <= 0.0f) return zero;
				if constexpr (ERROR == kErrorDiffuse) return display_sampling_error<V, kBiased>(p, pd, noise);
				for (uint32_t s = 0; s != S; ++s) {
					f3 dir = sample_psa<V, kBiased>(pd, next_noise_2(p, noise));
					float density = divide(dir.z, pd.total);
					dir = mul_transposed(world_to_shading, dir);
					add_light_mis_estimate<STRATEGY, RAYS, kTextured>(ctx, result, dir, density, sd, light);
				}
				density_factor = rcp(pd.total);
			}
		}
		else {
			// both techniques are prepared by the same code path (:506-547)
			if constexpr (ERROR == kErrorDiffuse || ERROR == kErrorSpecular) {
				psa_polygon<V> pd, ps;
				ps.total = 0.0f;
				ps.vertex_count = 0;
				ps.inner_ellipse_0 = mk2(0.0f, 0.0f);
				bool specular_culled = false;
#pragma unroll
				for (int t = 0; t != 2; ++t) {
					const m43& to_local = (t == 0) ? world_to_shading : world_to_cosine;
					if (t > 0) pd = ps;
					f3 vl[V];
#pragma unroll
					for (int j = 0; j < V - 1; ++j) vl[j] = mul_point(to_local, light_vertex(light, min((uint32_t) j, p.max_light_vertex_count - 1)));
					vl[V - 1] = zero;
					uint32_t clipped = clip_polygon<V>(count, vl);
					if (clipped == 0 && t == 0) return zero;
					else if (clipped == 0) { specular_culled = true; break; }
					prepare_psa<V, kBiased>(ps, clipped, vl);
				}
				if (specular_culled) ps.total = 0.0f;
				if (pd.total == 0.0f) return zero;
				if constexpr (ERROR == kErrorDiffuse) return display_sampling_error<V, kBiased>(p, pd, noise);
				if (ps.total > 0.0f) return display_sampling_error<V, kBiased>(p, ps, noise);
				return zero;
			}
			// The prepared polygons live in LDS (psa_compact, polygon_sampling.h): the diffuse one
			// first, then the specular one
			psa_compact<V> pd, ps;
			ps.total = 0.0f;
			ps.vertex_count = 0;
			ps.inner_slots = 0; ps.outer_slots = 0;
#pragma unroll
			for (int i = 0; i < V; ++i) ps.sector[i] = 0.0f;
			float2* const tables_d = ctx.psa_tables;
			// ... unless there is room for one table only (psa_table_in_memory(): V >= 6): then the specular polygon's table
			// is this thread's column of a table in device memory
			float2* const tables_s = psa_table_in_memory(V) ? ctx.psa_table_memory : ctx.psa_tables + kPsaTableSlots(V) * kPsaTableStride;
			constexpr bool kTerms = PREPARED == kPreparedLoadingTerms;
			// (with terms: this thread's quad of this light's diffuse and specular polygon, sector 0, half 0)
			const sector_terms_quad* const terms_d = kTerms ? ctx.terms + (size_t) ctx.light_index * kSectorTermQuads(V) * p.thread_count + ctx.tid : nullptr;
			const sector_terms_quad* const terms_s = kTerms ? terms_d + (size_t) sector_terms_quad_index(V, 1, 0u, 0) * p.thread_count : nullptr;
			if constexpr (PREPARED == kPreparedLoading || PREPARED == kPreparedLoadingTerms) {
				// (an earlier launch with the same inputs has left both polygons in device memory)
				if (!load_prepared<V>(ctx, pd, ps, tables_d, tables_s)) return zero;
			}
			else {
#pragma unroll
				for (int t = 0; t != 2; ++t) {
					const m43& to_local = (t == 0) ? world_to_shading : world_to_cosine;
					f3 vl[V];
#pragma unroll
					for (int j = 0; j < V - 1; ++j) vl[j] = mul_point(to_local, light_vertex(light, min((uint32_t) j, p.max_light_vertex_count - 1)));
					vl[V - 1] = zero;
					uint32_t clipped = clip_polygon<V>(count, vl);
					if (clipped == 0 && t == 0) {
						if constexpr (PREPARED == kPreparedStoring) store_prepared<V>(ctx, pd, ps, tables_d, tables_s, false);
						return zero;
					}
					else if (clipped == 0) break;  // the specular polygon is below the horizon: ps.total stays 0
					psa_polygon<V> prepared;
					prepare_psa<V, kBiased>(prepared, clipped, vl);
					if (t == 0) store_psa_tables<V>(pd, tables_d, prepared);
					else store_psa_tables<V>(ps, tables_s, prepared);
				}
				if constexpr (PREPARED == kPreparedStoring) store_prepared<V>(ctx, pd, ps, tables_d, tables_s, pd.total != 0.0f);
			}
			if (pd.total == 0.0f) return zero;
			float specular_albedo = ltc_in.albedo;
			float specular_weight = specular_albedo * ps.total;
			if constexpr (STRATEGY == kStrategySeparately) {
				for (uint32_t s = 0; s != S; ++s) {
					f3 dd;
					if constexpr (kTerms) {
						f2 u = next_noise_2(p, noise);
						dd = sample_psa_tables_with_terms<V, kBiased>(pd, tables_d, u, request_sector_terms<V>(pd, u.x, terms_d, p.thread_count));
					}
					else dd = sample_psa_tables<V, kBiased>(pd, tables_d, next_noise_2(p, noise));
					dd = mul_transposed(world_to_shading, dd);
					settle_noise(noise);
					float lambert;
					bool candidate;
					f3 rb = radiance_brdf<true, false, kTextured>(p, lambert, candidate, dd, sd, light);
					accumulate<RAYS>(ctx, result, candidate, rb * pd.total, zero * pd.total, dd, sd, light);
					if (ps.total > 0.0f) {
						f3 dc;
						if constexpr (kTerms) {
							f2 u = next_noise_2(p, noise);
							dc = sample_psa_tables_with_terms<V, kBiased>(ps, tables_s, u, request_sector_terms<V>(ps, u.x, terms_s, p.thread_count));
						}
						else dc = sample_psa_tables<V, kBiased>(ps, tables_s, next_noise_2(p, noise));
						f3 ds = normalize(cosine_to_shading(ltc_in, dc));
						float ltc_density = evaluate_ltc_density(ltc_in, ds, 1.0f);
						f3 dw = mul_transposed(world_to_shading, ds);
						f3 rb2 = radiance_brdf<false, true, kTextured>(p, lambert, candidate, dw, sd, light);
						if (!(ds.z <= 0.0f || dc.z <= 0.0f)) {
							f3 t = (rb2 * ds.z) * ps.total;
							f3 t0 = (zero * ds.z) * ps.total;
							accumulate<RAYS>(ctx, result, candidate, divide3(t, ltc_density), divide3(t0, ltc_density), dw, sd, light);
						}
						else if (RAYS == kRaysInline && candidate) {
							// the reference traces this ray even though the sample is discarded (:583-584)
							accumulate<RAYS>(ctx, result, candidate, zero, zero, dw, sd, light);
						}
					}
				}
			}
			else if constexpr (STRATEGY == kStrategyMis) {
				const int heuristic = p.mis_heuristic;
				const float visibility_estimate = load_f(p.constants, 156);
				f3 albedo = mk3(gmax(sd.diffuse_albedo.x, 0.01f), gmax(sd.diffuse_albedo.y, 0.01f), gmax(sd.diffuse_albedo.z, 0.01f));
				f3 diffuse_weight = albedo * pd.total;
				uint32_t technique_count = (ps.total > 0.0f) ? 2 : 1;
				float rcp_d = rcp(pd.total);
				float rcp_s = rcp(ps.total);
				f3 specular_weight_rgb = mk3(specular_weight, specular_weight, specular_weight);
				if (heuristic == kMisOptimal) {
					f3 radiance_over_pi = light_radiance(light) * kInvPi;
					diffuse_weight = diffuse_weight * radiance_over_pi;
					specular_weight_rgb = specular_weight_rgb * radiance_over_pi;
				}
				for (uint32_t s = 0; s != S; ++s) {
					f3 dir_d, dir_s = zero;
					if constexpr (kTerms) {
						// both random numbers are known here: both sectors are found and their four quads asked for before
						// either sample is drawn
						f2 u_d = next_noise_2(p, noise), u_s = mk2(0.0f, 0.0f);
						const psa_sector_request<V> request_d = request_sector_terms<V>(pd, u_d.x, terms_d, p.thread_count);
						if (ps.total > 0.0f) u_s = next_noise_2(p, noise);
						const psa_sector_request<V> request_s = request_sector_terms<V>(ps, u_s.x, terms_s, p.thread_count, ps.total > 0.0f);
						dir_d = sample_psa_tables_with_terms<V, kBiased>(pd, tables_d, u_d, request_d);
						if (ps.total > 0.0f) {
							dir_s = sample_psa_tables_with_terms<V, kBiased>(ps, tables_s, u_s, request_s);
							dir_s = normalize(cosine_to_shading(ltc_in, dir_s));
						}
					}
					else {
						dir_d = sample_psa_tables<V, kBiased>(pd, tables_d, next_noise_2(p, noise));
						if (ps.total > 0.0f) {
							dir_s = sample_psa_tables<V, kBiased>(ps, tables_s, next_noise_2(p, noise));
							dir_s = normalize(cosine_to_shading(ltc_in, dir_s));
						}
					}
					settle_noise(noise);
					for (uint32_t j = 0; j != technique_count; ++j) {
						f3 ds = (j == 0) ? dir_d : dir_s;
						if (ds.z <= 0.0f) continue;
						float dens_d = ds.z * rcp_d;
						float dens_s = evaluate_ltc_density(ltc_in, ds, rcp_s);
						float lambert;
						bool candidate;
						f3 dw = mul_transposed(world_to_shading, ds);
						f3 rb = radiance_brdf<true, true, kTextured>(p, lambert, candidate, dw, sd, light);
						f3 integrand = rb * ds.z;
						f3 dark = zero * ds.z;
						f3 visible_term, hidden_term;
						if (j == 0 && ps.total <= 0.0f) {
							visible_term = candidate ? integrand * rcp(dens_d) : zero;
							hidden_term = zero;
						}
						else if (j == 0) {
							mis_estimate_pair(heuristic, integrand, dark, diffuse_weight, dens_d, specular_weight_rgb, dens_s, visibility_estimate, visible_term, hidden_term);
						}
						else {
							mis_estimate_pair(heuristic, integrand, dark, specular_weight_rgb, dens_s, diffuse_weight, dens_d, visibility_estimate, visible_term, hidden_term);
						}
						accumulate<RAYS>(ctx, result, candidate, visible_term, hidden_term, dw, sd, light);
					}
				}
			}
			else if constexpr (STRATEGY == kStrategyRandom) {
				float lum = (sd.diffuse_albedo.x * 0.21263901f + sd.diffuse_albedo.y * 0.71516868f) + sd.diffuse_albedo.z * 0.07219232f;
				float diffuse_albedo = gmax(lum, 0.01f);
				float diffuse_weight = diffuse_albedo * pd.total;
				float diffuse_ratio = divide(diffuse_weight, diffuse_weight + specular_weight);
				for (uint32_t s = 0; s != S; ++s) {
					f2 u = next_noise_2(p, noise);
					bool specular_selected = u.x >= diffuse_ratio;
					float offset = specular_selected ? 1.0f : 0.0f;
					u.x = divide(u.x - offset, diffuse_ratio - offset);
					f3 ds;
					if constexpr (kTerms) {
						ds = specular_selected ? sample_psa_tables_with_terms<V, kBiased>(ps, tables_s, u, request_sector_terms<V>(ps, u.x, terms_s, p.thread_count))
							: sample_psa_tables_with_terms<V, kBiased>(pd, tables_d, u, request_sector_terms<V>(pd, u.x, terms_d, p.thread_count));
					}
					else ds = specular_selected ? sample_psa_tables<V, kBiased>(ps, tables_s, u) : sample_psa_tables<V, kBiased>(pd, tables_d, u);
					if (specular_selected) ds = normalize(cosine_to_shading(ltc_in, ds));
					settle_noise(noise);
					float lambert = ds.z;
					float dens_d = lambert * diffuse_albedo;
					float dens_s = evaluate_ltc_density(ltc_in, ds, specular_albedo);
					float density = divide(dens_d + dens_s, diffuse_weight + specular_weight);
					bool candidate;
					f3 dw = mul_transposed(world_to_shading, ds);
					f3 rb = radiance_brdf<true, true, kTextured>(p, lambert, candidate, dw, sd, light);
					if (!(ds.z <= 0.0f)) {
						f3 t = rb * ds.z;
						f3 t0 = zero * ds.z;
						accumulate<RAYS>(ctx, result, candidate, divide3(t, density), divide3(t0, density), dw, sd, light);
					}
					else if (RAYS == kRaysInline && candidate) accumulate<RAYS>(ctx, result, candidate, zero, zero, dw, sd, light);
				}
			}
		}
	}

	if constexpr (STRATEGY == kStrategyDiffuseGgxMis) {
		// GGX VNDF samples that happen to hit the light (:676-709)
		f3 out_shading = mul_direction(world_to_shading, sd.outgoing);
		out_shading.y = 0.0f;
		for (uint32_t s = 0; s != S; ++s) {
			float ggx_density;
			f3 dg = sample_ggx_reflected(ggx_density, out_shading, sd.roughness, next_noise_2(p, noise));
			f3 dw = mul_transposed(world_to_shading, dg);
			settle_noise(noise);
			if (dg.z > 0.0f && light_ray_intersection(light, p.max_light_vertex_count, sd.position, dw, 0.0f)) {
				float lambert;
				bool candidate;
				f3 rb = radiance_brdf<true, true, kTextured>(p, lambert, candidate, dw, sd, light);
				float polygon_density = kIsPsa ? (lambert * density_factor) : density_factor;
				float weight = mis_weight_over_density(p.mis_heuristic, ggx_density, polygon_density);
				accumulate<RAYS>(ctx, result, candidate, (rb * lambert) * weight, (zero * lambert) * weight, dw, sd, light);
			}
		}
	}
	if constexpr (is_deferred(RAYS)) {
		// close this light's run of terms; the resolve kernel scales by 1 / S and adds it
		if (ctx.light_clear && (ctx.final_state & 1u)) flush_final_sum(ctx);
		ctx.final_state = 2u;
		if (ctx.light_has_terms && ctx.code_cursor + 1 < p.max_codes) {
			if (ctx.noise) settle_noise(*ctx.noise);
			p.codes[code_slot(p.thread_count, ctx.code_cursor, ctx.tid)] = (uint8_t) kCodeEndOfLight;
			++ctx.code_cursor;
			ctx.light_has_terms = false;
		}
	}
	return result * (1.0f / (float) S);
}

// ---- the kernels --------------------------------------------------------------------------------

// main, shading_pass.frag.glsl:824-866
// (in the namespace of the arithmetic mode, like their launch properties: shade_params.h)
inline namespace VKR_MODE_NAMESPACE {
// Fills the sector terms of a launch from its kept polygons: one thread per (thread of the launch, light), grid
// (thread_count / 64, light_count), the tables of a pair in LDS as the shading kernel has them
template <int V>
__global__ void __launch_bounds__(kShadeThreads) k_sector_terms(const prepared_quad* prepared, sector_terms_quad* terms, uint32_t thread_count) {
	extern __shared__ float2 psa_tables[];
	const uint32_t tid = blockIdx.x * kShadeThreads + threadIdx.x, light = blockIdx.y;
	if (tid >= thread_count) return;
	float2* const tables_d = psa_tables + threadIdx.x;
	fill_sector_terms<V>(prepared + (size_t) light * kPreparedQuads(V) * thread_count + tid, terms + (size_t) light * kSectorTermQuads(V) * thread_count + tid, thread_count,
		tables_d, tables_d + kPsaTableSlots(V) * kPsaTableStride);
}
// the pointer that the storing and the loading instantiation get as their second argument; the plain one gets none
VKR_DEV prepared_quad* prepared_argument() { return nullptr; }
VKR_DEV prepared_quad* prepared_argument(prepared_quad* prepared) { return prepared; }
VKR_DEV prepared_quad* prepared_argument(prepared_quad* prepared, const sector_terms_quad*) { return prepared; }
VKR_DEV const sector_terms_quad* terms_argument() { return nullptr; }
VKR_DEV const sector_terms_quad* terms_argument(prepared_quad*) { return nullptr; }
VKR_DEV const sector_terms_quad* terms_argument(prepared_quad*, const sector_terms_quad* terms) { return terms; }
// PREPARED: kPreparedPlain - then BUFFER is empty and the kernel is the one that it always was -, or kPreparedStoring /
// kPreparedLoading where prepared_polygons_apply(), with the buffer of the prepared polygons as the second argument, or
// kPreparedLoadingTerms with the buffer of the sector terms as the third
template <int STRATEGY, int TECHNIQUE, int V, int RAYS, int ERROR = kErrorNone, int PREPARED = kPreparedPlain, typename... BUFFER>
__global__ void __launch_bounds__(kShadeThreads, shade_min_workgroups(STRATEGY, TECHNIQUE, V, RAYS, ERROR)) shade_pixels(const shade_params p, BUFFER... prepared) {
	static_assert(PREPARED == kPreparedPlain ? sizeof...(BUFFER) == 0 : (sizeof...(BUFFER) == (PREPARED == kPreparedLoadingTerms ? 2 : 1) && prepared_polygons_apply(STRATEGY, TECHNIQUE, V, RAYS, ERROR)), "no such variant");
	// A workgroup is ONE wave: the four 8x8 patches of a 16x16 block differ a lot in cost (background,
	// culled lights), and a wave that is done early gives its registers and LDS back at once instead
	// of waiting for its block (mean resident waves per SIMD 2.3 -> see profiles/).  Workgroup b runs
	// on XCD b % 8; the four patches of a block are the workgroups b, b + 8, b + 16, b + 24 of a
	// group of 32, so they share that XCD's L2.
	fill_atan_rows();  // (nothing outside the libm mode, device_math.h)
	const uint32_t b = blockIdx.x;
	const uint32_t local_block = ((b >> 5) << 3) | (b & 7u);
	const uint32_t block = p.first_block + local_block;
	const uint32_t thread = (((b >> 3) & 3u) << 6) | threadIdx.x;
	uint32_t px, py;
	size_t out_index;
	bool inside = local_block < p.block_count && locate_pixel(p, block, thread, px, py, out_index);
	// ray queue of this wave: one of the 64 queues of its XCD, so a queue counter's cache line is
	// only ever touched from one L2
	uint32_t queue = (b & 7u) * 64u + ((b >> 3) & 63u);
	// the polygon tables exist for the techniques that prepare two polygons per light in registers
	constexpr bool kTables = has_psa_tables(STRATEGY, TECHNIQUE, ERROR);
	// (dynamic LDS, shade_lds_bytes() at the launch: a static array would let the compiler conclude from
	// its size that a third wave cannot fit and drop the register limit that goes with three - at V = 7 ten
	// waves fit a CU, i.e. three on two of the four SIMDs)
	extern __shared__ float2 psa_tables[];
	// (the wavefront buffers are indexed by the thread's number within this launch)
	pixel_context ctx = {p};
	ctx.tid = local_block * 256u + thread;
	ctx.queue = queue;
	if constexpr (kTables) {
		ctx.psa_tables = psa_tables + threadIdx.x;
		if (psa_table_in_memory(V) && p.psa_table_memory) ctx.psa_table_memory = p.psa_table_memory + (size_t) b * (kPsaTableSlots(V) * kPsaTableStride) + threadIdx.x;
	}
	ctx.prepared = prepared_argument(prepared...);
	ctx.terms = terms_argument(prepared...);
	if constexpr (RAYS == kRaysDeferredBlocks) {
		// (the waves of a workgroup never touch each other's entry: no barrier)
		lds_state_word* state = ray_block_state();
		if ((threadIdx.x & 63u) == 0) { state[0] = 0; state[1] = 0; state[2] = 0; }
	}
	if (inside) {
		const uint8_t* c = p.constants;
		uint32_t primitive = p.visibility[(size_t) py * p.width + px];
		f3 color = mk3(0.0f, 0.0f, 0.0f);
		float fx = (float) (int32_t) px, fy = (float) (int32_t) py;
		f3 ray = mk3(
			(load_f(c, 96) * fx + load_f(c, 100) * fy) + load_f(c, 104) * 1.0f,
			(load_f(c, 112) * fx + load_f(c, 116) * fy) + load_f(c, 120) * 1.0f,
			(load_f(c, 128) * fx + load_f(c, 132) * fy) + load_f(c, 136) * 1.0f);
		shading_data sd;
		f3 end_xyz = ray;
		float end_w = 0.0f;
		if (primitive != 0xFFFFFFFFu) {
			sd = get_shading_data(p, primitive, ray, (size_t) py * p.width + px);
			end_xyz = sd.position;
			end_w = 1.0f;
			// every shadow ray of this pixel starts here
			if constexpr (is_deferred(RAYS)) p.ray_origins[ctx.tid] = make_float4(sd.position.x, sd.position.y, sd.position.z, 0.0f);
		}
		if (p.show_polygonal_lights) {
			f3 camera = load_f3(c, 144);
			f3 view_dir = normalize(ray);
			for (uint32_t i = 0; i != p.light_count; ++i) {
				light_ref light = get_light(p, i);
				if (light_ray_intersection(light, p.max_light_vertex_count, camera, end_xyz, end_w))
					color = color + polygon_radiance<ERROR != kErrorNone>(p, view_dir, camera, light);
			}
		}
		if (primitive != 0xFFFFFFFFu) {
			float fresnel_luminance = (sd.fresnel_0.x * 0.2126f + sd.fresnel_0.y * 0.7152f) + sd.fresnel_0.z * 0.0722f;
			ltc_coefficients ltc = get_ltc_coefficients(p, fresnel_luminance, sd.roughness, sd.position, sd.normal, sd.outgoing);
			noise_accessor noise = make_noise_accessor(p, px, py);
			ctx.noise = &noise;
			for (uint32_t i = 0; i != p.light_count; ++i) {
				light_ref light = get_light(p, i);
				if constexpr (is_deferred(RAYS)) {
					// the verdict of the shaft walk (light_shafts.h): 1 clear, 2 | n << 8 a list of n triangles, else trace
					uint32_t verdict = p.shaft_clear != nullptr ? *(constant_uint_pointer) (uintptr_t) (p.shaft_clear + ((size_t) b * p.light_count + i)) : 0u;
					bool listed = (verdict & 0xFFu) == 2u && p.shaft_lists != nullptr;
					ctx.light_clear = verdict == 1u || listed;
					ctx.list_count = listed ? ((verdict >> 8) & 0x1Fu) : 0u;
					ctx.list = p.shaft_lists + ((size_t) b * p.light_count + i) * (kShaftListMax * kShaftListEntry);
					ctx.light_index = i;
				}
				color = color + evaluate_light<STRATEGY, TECHNIQUE, V, RAYS, ERROR, PREPARED>(ctx, sd, ltc, light, noise);
			}
		}
		if constexpr (is_deferred(RAYS)) {
			// hand over to trace_shadow_rays / resolve_shadow_terms: the colour so far
			// (light display) and the terminated term stream
			// (without the light display the colour so far is +0, and the resolve kernel knows)
			if (p.show_polygonal_lights) p.base_color[ctx.tid] = make_float4(color.x, color.y, color.z, 0.0f);
			p.codes[code_slot(p.thread_count, ctx.code_cursor, ctx.tid)] = (uint8_t) kCodeEnd;
		}
		else
			store_final_color(p, out_index, color);
	}
	if constexpr (RAYS == kRaysDeferredBlocks) close_ray_block(p, queue);
	if (RAYS == kRaysInline && p.ray_counter) {
		// one atomic per wave
		uint32_t rays = ctx.rays;
#pragma unroll
		for (int offset = 32; offset > 0; offset >>= 1) rays += __shfl_xor(rays, offset);
		if ((threadIdx.x & 63) == 0 && rays) atomicAdd(p.ray_counter, (unsigned long long) rays);
	}
}

}  // inline namespace VKR_MODE_NAMESPACE

}  // namespace vkr
