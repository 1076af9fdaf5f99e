// What a build (bvh_build.hip) and a refit (bvh_refit.hip) must compute with the same operations, because a refit of
// unmoved vertices has to reproduce the build's bytes: the de-quantisation of a vertex, the box of a fragment of a split
// triangle and the order-preserving integer encoding of a float.  Device code, gfx950.
#pragma once
#include "lbvh.h"

namespace vkr {

// De-quantisation with two roundings (multiply, then add) like scene.c:176-187; the
// shading path uses a fused decode instead (mesh_quantization.glsl:38-45).
__device__ __forceinline__ f3 dequantize_position(uint2 q, const float (&factor)[3], const float (&summand)[3]) {
	float x = (float) (q.x & 0x1FFFFF);
	float y = (float) (((q.x & 0xFFE00000u) >> 21) | ((q.y & 0x3FF) << 11));
	float z = (float) ((q.y & 0x7FFFFC00u) >> 10);
	return mk3(__fadd_rn(__fmul_rn(x, factor[0]), summand[0]), __fadd_rn(__fmul_rn(y, factor[1]), summand[1]), __fadd_rn(__fmul_rn(z, factor[2]), summand[2]));
}

// Float minima / maxima as integer atomics: an encoding whose unsigned order is the order of the floats
__device__ __forceinline__ uint32_t ordered(float f) {
	uint32_t bits = __float_as_uint(f);
	return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
__device__ __forceinline__ float unordered(uint32_t u) {
	return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}

// What a leaf slot remembers of the fragment it was built for (acceleration_structure_t.leaf_fragments): slab j of count
// slabs of its triangle, count == 1 for a whole triangle
constexpr uint32_t kMostFragments = 16;
__host__ __device__ __forceinline__ uint32_t pack_leaf_fragment(uint32_t j, uint32_t count) { return (j << 16) | count; }

// the longest axis of a box, x before y before z
__device__ __forceinline__ int longest_axis(f3 lo, f3 hi) {
	f3 e = hi - lo;
	return (e.x >= e.y && e.x >= e.z) ? 0 : (e.y >= e.z ? 1 : 2);
}

// bounds of the part of the triangle with s0 <= x_axis <= s1 (the triangle is cut by the two planes)
__device__ __forceinline__ void slab_bounds(const f3 (&v)[3], int axis, float s0, float s1, f3& lo, f3& hi) {
	float px[8], py[8], pz[8], qx[8], qy[8], qz[8];
	int count = 3;
	for (int i = 0; i != 3; ++i) { px[i] = v[i].x; py[i] = v[i].y; pz[i] = v[i].z; }
	for (int side = 0; side != 2; ++side) {
		// keep x_axis >= s0 (side 0), x_axis <= s1 (side 1)
		float plane = side ? s1 : s0, sign = side ? -1.0f : 1.0f;
		int kept = 0;
		for (int i = 0; i != count; ++i) {
			int j = (i + 1 == count) ? 0 : i + 1;
			float ci = axis == 0 ? px[i] : (axis == 1 ? py[i] : pz[i]), cj = axis == 0 ? px[j] : (axis == 1 ? py[j] : pz[j]);
			float di = sign * (ci - plane), dj = sign * (cj - plane);
			if (di >= 0.0f) { qx[kept] = px[i]; qy[kept] = py[i]; qz[kept] = pz[i]; ++kept; }
			if ((di >= 0.0f) != (dj >= 0.0f)) {
				float w = di / (di - dj);
				qx[kept] = fmaf(w, px[j] - px[i], px[i]); qy[kept] = fmaf(w, py[j] - py[i], py[i]); qz[kept] = fmaf(w, pz[j] - pz[i], pz[i]);
				// (the point lies on the plane: say so exactly, whatever the interpolation rounded to)
				if (axis == 0) qx[kept] = plane; else if (axis == 1) qy[kept] = plane; else qz[kept] = plane;
				++kept;
			}
		}
		count = kept;
		for (int i = 0; i != count; ++i) { px[i] = qx[i]; py[i] = qy[i]; pz[i] = qz[i]; }
	}
	lo = mk3(3.0e38f, 3.0e38f, 3.0e38f); hi = mk3(-3.0e38f, -3.0e38f, -3.0e38f);
	for (int i = 0; i != count; ++i) {
		lo = mk3(fminf(lo.x, px[i]), fminf(lo.y, py[i]), fminf(lo.z, pz[i]));
		hi = mk3(fmaxf(hi.x, px[i]), fmaxf(hi.y, py[i]), fmaxf(hi.z, pz[i]));
	}
}

// The box of fragment j of count > 1 of the triangle v with the box [lo, hi]: the part of the triangle inside slab j along `axis`
__device__ __forceinline__ void fragment_bounds(const f3 (&v)[3], f3 lo, f3 hi, int axis, uint32_t j, uint32_t count, f3& flo, f3& fhi) {
	float a0 = axis == 0 ? lo.x : (axis == 1 ? lo.y : lo.z), a1 = axis == 0 ? hi.x : (axis == 1 ? hi.y : hi.z);
	// (the planes between the slabs are shared: slab j ends where slab j + 1 begins, bit for bit)
	float s0 = j == 0u ? a0 : fmaf((float) j / (float) count, a1 - a0, a0);
	float s1 = j + 1u == count ? a1 : fmaf((float) (j + 1u) / (float) count, a1 - a0, a0);
	slab_bounds(v, axis, s0, s1, flo, fhi);
	// a slab that the clipping left empty (rounding at the ends) keeps a point of the triangle's box
	if (!(flo.x <= fhi.x)) { flo = lo; fhi = lo; }
	// never beyond the triangle's own box
	flo = mk3(fmaxf(flo.x, lo.x), fmaxf(flo.y, lo.y), fmaxf(flo.z, lo.z));
	fhi = mk3(fminf(fhi.x, hi.x), fminf(fhi.y, hi.y), fminf(fhi.z, hi.z));
}

// One axis of an fp32 box on the 15-bit grid, rounded outwards by kGridMargin and clamped: lo | hi << 16 (lbvh.h)
__device__ __forceinline__ uint32_t quantize_box_axis(float lo, float hi, float origin, float inverse_cell) {
	float q0 = floorf((lo - origin) * inverse_cell - kGridMargin);
	float q1 = ceilf((hi - origin) * inverse_cell + kGridMargin);
	q0 = fminf(fmaxf(q0, 0.0f), kGridMax);
	q1 = fminf(fmaxf(q1, 0.0f), kGridMax);
	return (uint32_t) q0 | ((uint32_t) q1 << 16);
}

}  // namespace vkr
