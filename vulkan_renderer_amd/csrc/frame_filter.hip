// Frame filter (include/vkr_frame_filter.h): the edge-avoiding a-trous wavelet with a variance-guided luminance weight.
// One launch per iteration; the first prepares (modulation, variance scale), the last finishes.  Compiled without
// contraction in the exact mode's flags, whatever the arithmetic mode of the pass; every result is restated in numpy bit
// for bit (vulkan_renderer_amd/frame_filter.py).
#include "vkr_frame_filter.h"
#include "frame_images.h"

using namespace vkr;

// ---- kernel ------------------------------------------------------------------------------------------------------

// One iteration: where it reads and writes (modulation: NULL unless the launch prepares or finishes; variance and
// out_variance: NULL when not wanted; all wave-uniform) and the settings
struct filter_iteration {
	const float4 *colour, *variance, *position, *normal, *modulation;
	float4 *out_colour, *out_variance;
	uint32_t width, height;
	int32_t step;
	uint32_t normal_squarings;
	float sigma_luminance, sigma_depth, variance_scale;
};

VKR_DEV float luminance(f3 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }

// What the taps of a pixel are weighed against
struct filter_centre {
	f3 P, n;
	float l, d_z, d_l;
};

// sum_c, sum_v and sum_w of the header
struct filter_sums {
	f3 c, v;
	float w;
};

// d_l of the header from the sums of the 3x3 Gaussian of the variance
VKR_DEV float luminance_scale(const filter_iteration& f, f3 sum_gv, float sum_g) {
	f3 vbar = mk3(divide_full_range(sum_gv.x, sum_g), divide_full_range(sum_gv.y, sum_g), divide_full_range(sum_gv.z, sum_g));
	return f.sigma_luminance * luminance(mk3(__builtin_sqrtf(vbar.x), __builtin_sqrtf(vbar.y), __builtin_sqrtf(vbar.z))) + 1.0e-8f;
}

// w of a tap other than the centre that is in the frame and covered; 0 where the rule skips it.  A tap whose normal leaves it
// no weight (h * w_n not > 0) returns early, which changes no bit: its w would not be > 0 either.
template <bool VARIANCE> VKR_DEV float tap_weight(const filter_iteration& f, const filter_centre& p, float h, f3 P_q, f3 n_q, f3 c_q) {
	float w_n = gmax(0.0f, dot(p.n, n_q));
	for (uint32_t k = 0; k != f.normal_squarings; ++k) w_n = w_n * w_n;
	float hn = h * w_n;
	if (!(hn > 0.0f)) return 0.0f;
	// (e_z + 0 is e_z in every bit: without a variance image the luminance term is left out)
	float e = divide_full_range(fabsf(dot(p.n, P_q - p.P)), p.d_z);
	if (VARIANCE) e = e + divide_full_range(fabsf(luminance(c_q) - p.l), p.d_l);
	float t = -e * 1.44269502f;
	// (a NaN fails the comparison)
	float w_e = (t >= -126.0f) ? exp2_poly(t) : 0.0f;
	float w = hn * w_e;
	return (w > 0.0f) ? w : 0.0f;
}

template <bool VARIANCE> VKR_DEV void add_tap(filter_sums& sums, float w, f3 c_q, f3 v_q) {
	sums.c = sums.c + c_q * w;
	if (VARIANCE) sums.v = sums.v + v_q * (w * w);
	sums.w = sums.w + w;
}

VKR_DEV float kernel_weight(int dx, int dy) {
	const float kx = (dx == 0) ? 0.375f : ((dx == 1 || dx == -1) ? 0.25f : 0.0625f);
	const float ky = (dy == 0) ? 0.375f : ((dy == 1 || dy == -1) ? 0.25f : 0.0625f);
	return kx * ky;
}

// c' and v' of a covered pixel from its sums, finished in the last launch; alpha: the bits of the input's
template <bool LAST, bool VARIANCE> VKR_DEV void store_filtered(const filter_iteration& f, size_t p, const filter_sums& sums, float alpha) {
	f3 c = mk3(divide_full_range(sums.c.x, sums.w), divide_full_range(sums.c.y, sums.w), divide_full_range(sums.c.z, sums.w));
	f3 m = mk3(1.0f, 1.0f, 1.0f);
	const bool modulated = LAST && f.modulation;
	if (modulated) {
		m = modulation_of(f.modulation[p]);
		c = c * m;
	}
	f.out_colour[p] = make_float4(c.x, c.y, c.z, alpha);
	if (VARIANCE && f.out_variance) {
		float square = sums.w * sums.w;
		f3 v = mk3(divide_full_range(sums.v.x, square), divide_full_range(sums.v.y, square), divide_full_range(sums.v.z, square));
		if (modulated) v = v * (m * m);
		f.out_variance[p] = make_float4(v.x, v.y, v.z, 1.0f);
	}
}

// ---- the first launch: step 1 and the prepare, from an LDS tile ---------------------------------------------------

// The tile of a workgroup with its halo of two pixels.  Rows are 24 pixels apart: a ds_read_b128 is served in four groups
// of sixteen lanes - of an 8x8 wave, half rows of four rows - and with 24 (8 mod 16) the sixteen 16-byte slots of every
// group are distinct (with 20 two of the four half rows of a group fall on the same four slots).
constexpr int kHalo = 2, kTileExtent = 16 + 2 * kHalo, kTileStride = 24, kTileSlots = kTileExtent * kTileStride;

// Every pixel of the tile is prepared once - with a modulation image six full-range quotients, which a launch that prepares
// per tap pays 25 + 9 times per pixel - and the 24 taps and 8 variance neighbours of step 1 come from LDS.  A tile pixel out
// of the frame has distance 0 like one that is not covered: neither is a tap.  Serves every extent (a frame smaller than
// the tile fills less of it).  position.xyz | distance, normal.xyz, c0.rgb | alpha, v0.rgb: 4 x 7.5 KB.
template <bool LAST, bool VARIANCE>
__global__ void __launch_bounds__(256) k_filter_first_iteration(const filter_iteration f) {
	__shared__ float4 tile_position[kTileSlots], tile_normal[kTileSlots], tile_colour[kTileSlots], tile_variance[VARIANCE ? kTileSlots : 1];
	const int32_t x0 = (int32_t) (blockIdx.x * 16) - kHalo, y0 = (int32_t) (blockIdx.y * 16) - kHalo;
	for (uint32_t i = threadIdx.x; i < (uint32_t) (kTileExtent * kTileExtent); i += 256) {
		uint32_t ty = i / kTileExtent, tx = i - ty * kTileExtent;
		int32_t qx = x0 + (int32_t) tx, qy = y0 + (int32_t) ty;
		const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		float4 position = zero, normal = zero, colour = zero, variance = zero;
		if ((uint32_t) qx < f.width && (uint32_t) qy < f.height) {
			size_t q = (size_t) qy * f.width + (size_t) qx;
			position = f.position[q];
			normal = f.normal[q];
			colour = f.colour[q];
			if (VARIANCE) variance = f.variance[q];
			f3 c = rgb(colour), v = rgb(variance) * f.variance_scale;
			if (f.modulation) {
				f3 m = modulation_of(f.modulation[q]);
				c = divide3_full_range(c, m);
				if (VARIANCE) v = divide3_full_range(v, m * m);
			}
			colour = make_float4(c.x, c.y, c.z, colour.w);
			variance = make_float4(v.x, v.y, v.z, 0.0f);
		}
		uint32_t slot = ty * kTileStride + tx;
		tile_position[slot] = position;
		tile_normal[slot] = normal;
		tile_colour[slot] = colour;
		if (VARIANCE) tile_variance[slot] = variance;
	}
	__syncthreads();
	uint32_t lx, ly;
	lane_pixel(lx, ly);
	uint32_t px = blockIdx.x * 16 + lx, py = blockIdx.y * 16 + ly;
	if (px >= f.width || py >= f.height) return;
	size_t p = (size_t) py * f.width + px;
	const uint32_t own = (ly + kHalo) * kTileStride + lx + kHalo;
	float4 position_p = tile_position[own];
	if (!(position_p.w > 0.0f)) {
		// not covered: the bytes pass through as they are
		f.out_colour[p] = f.colour[p];
		if (VARIANCE && f.out_variance) f.out_variance[p] = f.variance[p];
		return;
	}
	float4 colour_p = tile_colour[own];
	f3 c_p = rgb(colour_p), v_p = VARIANCE ? rgb(tile_variance[own]) : mk3(0.0f, 0.0f, 0.0f);
	filter_centre centre;
	centre.P = rgb(position_p);
	centre.n = rgb(tile_normal[own]);
	centre.l = luminance(c_p);
	centre.d_z = f.sigma_depth * position_p.w;
	centre.d_l = 0.0f;
	if (VARIANCE) {
		f3 sum_gv = mk3(0.0f, 0.0f, 0.0f);
		float sum_g = 0.0f;
#pragma unroll
		for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
			for (int dx = -1; dx <= 1; ++dx) {
				const float g = ((dx == 0) ? 0.5f : 0.25f) * ((dy == 0) ? 0.5f : 0.25f);
				const uint32_t q = (uint32_t) ((int32_t) own + dy * kTileStride + dx);
				if ((dx != 0 || dy != 0) && !(tile_position[q].w > 0.0f)) continue;
				sum_gv = sum_gv + rgb(tile_variance[q]) * g;
				sum_g = sum_g + g;
			}
		}
		centre.d_l = luminance_scale(f, sum_gv, sum_g);
	}
	filter_sums sums = {mk3(0.0f, 0.0f, 0.0f), mk3(0.0f, 0.0f, 0.0f), 0.0f};
#pragma unroll
	for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
		for (int dx = -2; dx <= 2; ++dx) {
			const float h = kernel_weight(dx, dy);
			if (dx == 0 && dy == 0) {
				add_tap<VARIANCE>(sums, h, c_p, v_p);
				continue;
			}
			const uint32_t q = (uint32_t) ((int32_t) own + dy * kTileStride + dx);
			float4 position_q = tile_position[q];
			if (!(position_q.w > 0.0f)) continue;
			f3 c_q = rgb(tile_colour[q]);
			float w = tap_weight<VARIANCE>(f, centre, h, rgb(position_q), rgb(tile_normal[q]), c_q);
			if (!(w > 0.0f)) continue;
			add_tap<VARIANCE>(sums, w, c_q, VARIANCE ? rgb(tile_variance[q]) : v_p);
		}
	}
	store_filtered<LAST, VARIANCE>(f, p, sums, colour_p.w);
}

// ---- the later launches: steps 2, 4, 8, 16 from global memory -----------------------------------------------------

// What an iteration reads of a pixel (variance: with a variance image only)
struct filter_pixel {
	float4 position, normal, colour, variance;
};

template <bool VARIANCE> VKR_DEV filter_pixel load_pixel(const filter_iteration& f, size_t i) {
	filter_pixel q = {};
	q.position = f.position[i];
	q.normal = f.normal[i];
	q.colour = f.colour[i];
	if (VARIANCE) q.variance = f.variance[i];
	return q;
}

// Plain global loads: neighbouring waves and workgroups read the same lines, which the caches serve at every step (measured:
// steps 2, 4 and 8 take the same time).  The loads of a row of five taps are issued together, whatever the guides will say
// of the taps (a column out of the frame reads the lane's own column instead and is not used): twenty loads in flight per
// lane instead of four that wait for each other.  The arithmetic of a tap runs only where the tap is in the frame and covered.
template <bool LAST, bool VARIANCE>
__global__ void __launch_bounds__(256) k_filter_iteration(const filter_iteration f) {
	uint32_t lx, ly;
	lane_pixel(lx, ly);
	uint32_t px = blockIdx.x * 16 + lx, py = blockIdx.y * 16 + ly;
	if (px >= f.width || py >= f.height) return;
	size_t p = (size_t) py * f.width + px;
	const filter_pixel own = load_pixel<VARIANCE>(f, p);
	if (!(own.position.w > 0.0f)) {
		// not covered: the bytes pass through every iteration as they are
		f.out_colour[p] = own.colour;
		if (VARIANCE && f.out_variance) f.out_variance[p] = own.variance;
		return;
	}
	f3 c_p = rgb(own.colour), v_p = rgb(own.variance);
	filter_centre centre;
	centre.P = rgb(own.position);
	centre.n = rgb(own.normal);
	centre.l = luminance(c_p);
	centre.d_z = f.sigma_depth * own.position.w;
	centre.d_l = 0.0f;
	if (VARIANCE) {
		f3 sum_gv = mk3(0.0f, 0.0f, 0.0f);
		float sum_g = 0.0f;
#pragma unroll
		for (int dy = -1; dy <= 1; ++dy) {
			int32_t qy = (int32_t) py + dy;
			if ((uint32_t) qy >= f.height) continue;
			size_t row = (size_t) qy * f.width;
			float distance[3] = {};
			float4 variance[3] = {};
			bool inside[3] = {};
#pragma unroll
			for (int dx = -1; dx <= 1; ++dx) {
				if (dx == 0 && dy == 0) continue;
				int32_t qx = (int32_t) px + dx;
				inside[dx + 1] = (uint32_t) qx < f.width;
				size_t q = row + (size_t) (inside[dx + 1] ? qx : (int32_t) px);
				distance[dx + 1] = f.position[q].w;
				variance[dx + 1] = f.variance[q];
			}
#pragma unroll
			for (int dx = -1; dx <= 1; ++dx) {
				const float g = ((dx == 0) ? 0.5f : 0.25f) * ((dy == 0) ? 0.5f : 0.25f);
				f3 v_q = v_p;
				if (dx != 0 || dy != 0) {
					if (!inside[dx + 1] || !(distance[dx + 1] > 0.0f)) continue;
					v_q = rgb(variance[dx + 1]);
				}
				sum_gv = sum_gv + v_q * g;
				sum_g = sum_g + g;
			}
		}
		centre.d_l = luminance_scale(f, sum_gv, sum_g);
	}
	filter_sums sums = {mk3(0.0f, 0.0f, 0.0f), mk3(0.0f, 0.0f, 0.0f), 0.0f};
#pragma unroll
	for (int dy = -2; dy <= 2; ++dy) {
		int32_t qy = (int32_t) py + dy * f.step;
		if ((uint32_t) qy >= f.height) continue;
		size_t row = (size_t) qy * f.width;
		filter_pixel taps[5] = {};
		bool inside[5] = {};
#pragma unroll
		for (int dx = -2; dx <= 2; ++dx) {
			if (dx == 0 && dy == 0) continue;
			int32_t qx = (int32_t) px + dx * f.step;
			inside[dx + 2] = (uint32_t) qx < f.width;
			taps[dx + 2] = load_pixel<VARIANCE>(f, row + (size_t) (inside[dx + 2] ? qx : (int32_t) px));
		}
#pragma unroll
		for (int dx = -2; dx <= 2; ++dx) {
			const float h = kernel_weight(dx, dy);
			if (dx == 0 && dy == 0) {
				add_tap<VARIANCE>(sums, h, c_p, v_p);
				continue;
			}
			const filter_pixel& q = taps[dx + 2];
			if (!inside[dx + 2] || !(q.position.w > 0.0f)) continue;
			f3 c_q = rgb(q.colour);
			float w = tap_weight<VARIANCE>(f, centre, h, rgb(q.position), rgb(q.normal), c_q);
			if (!(w > 0.0f)) continue;
			add_tap<VARIANCE>(sums, w, c_q, rgb(q.variance));
		}
	}
	store_filtered<LAST, VARIANCE>(f, p, sums, own.colour.w);
}

template <bool VARIANCE> static void launch_iteration(const filter_iteration& f, bool first, bool last, hipStream_t stream) {
	dim3 grid((f.width + 15) / 16, (f.height + 15) / 16);
	if (first && last) k_filter_first_iteration<true, VARIANCE><<<grid, 256, 0, stream>>>(f);
	else if (first) k_filter_first_iteration<false, VARIANCE><<<grid, 256, 0, stream>>>(f);
	else if (last) k_filter_iteration<true, VARIANCE><<<grid, 256, 0, stream>>>(f);
	else k_filter_iteration<false, VARIANCE><<<grid, 256, 0, stream>>>(f);
}

// ---- host side ---------------------------------------------------------------------------------------------------

// The two pairs of scratch images that the iterations alternate between, and the event behind the last one
static frame_image_set images_of(frame_filter_t* filter) {
	return {"filter", &filter->width, &filter->height, &filter->filtered, 4,
		{&filter->colour_scratch[0], &filter->colour_scratch[1], &filter->variance_scratch[0], &filter->variance_scratch[1]}};
}

extern "C" void destroy_frame_filter(frame_filter_t* filter, application_t* app) {
	destroy_frame_images(images_of(filter), app);
	memset(filter, 0, sizeof(*filter));
}

extern "C" int create_frame_filter(frame_filter_t* filter, application_t* app, uint32_t width, uint32_t height) {
	memset(filter, 0, sizeof(*filter));
	return create_frame_images(images_of(filter), app, width, height, VKR_FRAME_FILTER_MAX_EXTENT, false, "scratch images");
}

extern "C" int filter_frame(frame_filter_t* filter, application_t* app, const frame_filter_settings_t* settings, const frame_filter_images_t* images) {
	if (!filter || !app || !settings || !images) {
		printf("filter_frame() needs a filter, an application, settings and images.\n");
		return 1;
	}
	// (written so that a NaN fails)
	if (settings->iteration_count < 1 || settings->iteration_count > VKR_FRAME_FILTER_MAX_ITERATIONS || settings->normal_squarings > VKR_FRAME_FILTER_MAX_NORMAL_SQUARINGS
		|| !(settings->sigma_luminance > 0.0f && settings->sigma_luminance < INFINITY) || !(settings->sigma_depth > 0.0f && settings->sigma_depth < INFINITY)
		|| !(settings->variance_scale >= 0.0f && settings->variance_scale < INFINITY))
	{
		printf("filter_frame() takes 1 to %d iterations, 0 to %d squarings of the normal weight, finite sigmas > 0 and a finite variance scale >= 0.\n", VKR_FRAME_FILTER_MAX_ITERATIONS, VKR_FRAME_FILTER_MAX_NORMAL_SQUARINGS);
		return 1;
	}
	if (images->out_variance && !images->variance) {
		printf("filter_frame(): a variance output needs a variance image.\n");
		return 1;
	}
	const frame_call call = {"filter_frame", {images->colour, images->variance, images->position, images->normal, images->modulation}, {images->out_colour, images->out_variance}};
	if (check_frame_call_images(call, images->colour && images->position && images->normal && images->out_colour)) return 1;
	const frame_image_set own = images_of(filter);
	if (!frame_images_created(own)) {
		printf("filter_frame() needs a filter created by create_frame_filter().\n");
		return 1;
	}
	const size_t bytes = frame_image_bytes(own);
	hipStream_t stream;
	if (check_frame_call_overlap(call, bytes, NULL) || begin_frame_call(call, app, bytes, &stream)) return 1;
	const uint32_t n = settings->iteration_count;
	for (uint32_t i = 0; i != n; ++i) {
		const bool first = i == 0, last = i + 1 == n;
		filter_iteration f;
		f.colour = (const float4*) (first ? images->colour : filter->colour_scratch[(i - 1) & 1]);
		f.variance = (const float4*) (!images->variance ? NULL : (first ? images->variance : filter->variance_scratch[(i - 1) & 1]));
		f.position = (const float4*) images->position;
		f.normal = (const float4*) images->normal;
		f.modulation = (const float4*) ((first || last) ? images->modulation : NULL);
		f.out_colour = (float4*) (last ? images->out_colour : filter->colour_scratch[i & 1]);
		f.out_variance = (float4*) (!images->variance ? NULL : (last ? images->out_variance : filter->variance_scratch[i & 1]));
		f.width = filter->width;
		f.height = filter->height;
		f.step = (int32_t) (1u << i);
		f.normal_squarings = settings->normal_squarings;
		f.sigma_luminance = settings->sigma_luminance;
		f.sigma_depth = settings->sigma_depth;
		f.variance_scale = settings->variance_scale;
		if (images->variance) launch_iteration<true>(f, first, last, stream);
		else launch_iteration<false>(f, first, last, stream);
		if (hip_failed(hipGetLastError(), "filtering a frame")) return 1;
	}
	return finish_frame_call(call, app, bytes, filter->filtered, "marking the filtered frame");
}
