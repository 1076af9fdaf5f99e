// Frame history (include/vkr_frame_history.h): the frame blended into a history that is fetched where each pixel was under
// the previous camera - or, with the images of render_motion_buffers(), where its surface was -, and the variance of the
// result.  One launch accumulates; a second one replaces the variance of pixels with a short history by a spatial estimate.  Compiled without contraction in the exact mode's flags, whatever the
// arithmetic mode of the pass; every result is restated in numpy bit for bit (vulkan_renderer_amd/frame_history.py).
#include "vkr_frame_history.h"
#include "frame_images.h"

using namespace vkr;

// ---- kernels -----------------------------------------------------------------------------------------------------

// One call: the caller's images (reprojection, modulation, previous_position, out_variance: NULL when not given), the set h
// that is read (only with has_history) and the set h' that is written, and the settings.  All wave-uniform.
struct history_frame {
	const float4 *colour, *position, *normal, *reprojection, *modulation, *previous_position;
	const float4 *old_colour, *old_moments, *old_position, *old_normal;
	float4 *new_colour, *new_moments, *new_position, *new_normal;
	float4 *out_colour, *out_variance;
	uint32_t width, height, has_history;
	float max_length, sigma_depth, normal_threshold, spatial_length;
};

// Whether a pixel at P_q with normal n_q belongs to the surface of p: the plane test and the normal test of the header
VKR_DEV bool same_surface(const history_frame& f, f3 P_p, f3 n_p, float d_z, f3 P_q, f3 n_q) {
	if (!(fabsf(dot(n_p, P_q - P_p)) <= d_z)) return false;
	return dot(n_p, n_q) >= f.normal_threshold;
}

// The sixteen loads of the four taps are issued together, before the verdict on any of them (a tap out of the frame, and
// every tap of a pixel that is not usable, reads the lane's own pixel and is not used): sixteen loads in flight per lane
// instead of four chains of four.  The first frame of a history reads no history at all.  MOVING
// (accumulate_moving_frame_history()): the taps' positions are compared with where the pixel's surface was, one more load.
template <bool VARIANCE, bool MOVING>
__global__ void __launch_bounds__(256) k_accumulate_history(const history_frame f) {
	uint32_t lx, ly;
	lane_pixel(lx, ly);
	uint32_t px = blockIdx.x * 16 + lx, py = blockIdx.y * 16 + ly;
	if (px >= f.width || py >= f.height) return;
	const size_t p = (size_t) py * f.width + px;
	const float4 position_p = f.position[p], normal_p = f.normal[p], colour_p = f.colour[p];
	float4 r = make_float4((float) px, (float) py, 1.0f, 1.0f);
	if (f.reprojection) r = f.reprojection[p];
	f3 m = mk3(1.0f, 1.0f, 1.0f);
	if (f.modulation) m = modulation_of(f.modulation[p]);
	f.new_position[p] = position_p;
	f.new_normal[p] = normal_p;
	if (!(position_p.w > 0.0f)) {
		const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		f.new_colour[p] = zero;
		f.new_moments[p] = zero;
		f.out_colour[p] = colour_p;
		if (VARIANCE) f.out_variance[p] = zero;
		return;
	}
	// (nothing of r is trusted: only coordinates that passed these bounds become integers)
	const bool usable = f.has_history && r.w == 1.0f && r.x >= -1.0f && r.x < (float) f.width && r.y >= -1.0f && r.y < (float) f.height;
	f3 sum_c = mk3(0.0f, 0.0f, 0.0f), sum_s = mk3(0.0f, 0.0f, 0.0f);
	float sum_b = 0.0f, sum_n = 0.0f;
	if (f.has_history) {
		const float X = usable ? r.x : (float) px, Y = usable ? r.y : (float) py;
		const float floor_x = floorf(X), floor_y = floorf(Y);
		const float tx = X - floor_x, ty = Y - floor_y;
		const int32_t fx = (int32_t) floor_x, fy = (int32_t) floor_y;
		float4 tap_position[4], tap_normal[4], tap_colour[4], tap_moments[4];
		bool inside[4];
#pragma unroll
		for (int k = 0; k != 4; ++k) {
			const int32_t qx = fx + (k & 1), qy = fy + (k >> 1);
			inside[k] = (uint32_t) qx < f.width && (uint32_t) qy < f.height;
			const size_t q = inside[k] ? (size_t) qy * f.width + (size_t) qx : p;
			tap_position[k] = f.old_position[q];
			tap_normal[k] = f.old_normal[q];
			tap_colour[k] = f.old_colour[q];
			tap_moments[k] = f.old_moments[q];
		}
		f3 P_p = rgb(position_p);
		if (MOVING) P_p = rgb(f.previous_position[p]);
		const f3 n_p = rgb(normal_p);
		const float d_z = f.sigma_depth * position_p.w;
#pragma unroll
		for (int k = 0; k != 4; ++k) {
			const float bx = (k & 1) ? tx : 1.0f - tx, by = (k >> 1) ? ty : 1.0f - ty;
			const float b = bx * by;
			if (!usable || !inside[k] || !(b > 0.0f) || !(tap_position[k].w > 0.0f)) continue;
			if (!same_surface(f, P_p, n_p, d_z, rgb(tap_position[k]), rgb(tap_normal[k]))) continue;
			sum_b = sum_b + b;
			sum_c = sum_c + rgb(tap_colour[k]) * b;
			sum_s = sum_s + rgb(tap_moments[k]) * b;
			sum_n = sum_n + tap_colour[k].w * b;
		}
	}
	f3 c = rgb(colour_p);
	if (f.modulation) c = divide3_full_range(c, m);
	const f3 s = c * c;
	const bool finite = fabsf(c.x) < INFINITY && fabsf(c.y) < INFINITY && fabsf(c.z) < INFINITY;
	f3 new_c = mk3(0.0f, 0.0f, 0.0f), new_s = mk3(0.0f, 0.0f, 0.0f);
	float new_n = 0.0f;
	if (usable && sum_b >= 1.0f / 64.0f) {
		const f3 hc = divide3_full_range(sum_c, sum_b), hs = divide3_full_range(sum_s, sum_b);
		const float n = divide_full_range(sum_n, sum_b);
		new_c = hc;
		new_s = hs;
		new_n = n;
		if (finite) {
			new_n = gmin(n + 1.0f, f.max_length);
			const float a = divide_full_range(1.0f, new_n);
			new_c = hc + (c - hc) * a;
			new_s = hs + (s - hs) * a;
		}
	}
	else if (finite) {
		new_c = c;
		new_s = s;
		new_n = 1.0f;
	}
	f.new_colour[p] = make_float4(new_c.x, new_c.y, new_c.z, new_n);
	f.new_moments[p] = make_float4(new_s.x, new_s.y, new_s.z, 0.0f);
	f3 out = new_c;
	if (f.modulation) out = out * m;
	f.out_colour[p] = make_float4(out.x, out.y, out.z, colour_p.w);
	if (VARIANCE) {
		f3 v = gmax3(0.0f, new_s - new_c * new_c) * divide_full_range(1.0f, gmax(new_n, 1.0f));
		if (f.modulation) v = v * (m * m);
		f.out_variance[p] = make_float4(v.x, v.y, v.z, 1.0f);
	}
}

// The spatial estimate for pixels with a short history, from the set that k_accumulate_history just wrote.  A lane whose
// length is not in 0 < n' < spatial_length leaves after one four-byte load (an uncovered pixel has n' = 0, so a length
// above 0 says that p is covered); once a camera stands still that is every lane of every wave.  The others take the loads
// of a row of seven pixels together, as the frame filter does, and plain global loads: neighbours read the same lines.
__global__ void __launch_bounds__(256) k_history_spatial_variance(const history_frame f) {
	uint32_t lx, ly;
	lane_pixel(lx, ly);
	uint32_t px = blockIdx.x * 16 + lx, py = blockIdx.y * 16 + ly;
	if (px >= f.width || py >= f.height) return;
	const size_t p = (size_t) py * f.width + px;
	const float n_p_length = f.new_colour[p].w;
	if (!(n_p_length > 0.0f && n_p_length < f.spatial_length)) return;
	const float4 position_p = f.position[p];
	const f3 P_p = rgb(position_p), n_p = rgb(f.normal[p]);
	const float d_z = f.sigma_depth * position_p.w;
	f3 M1 = mk3(0.0f, 0.0f, 0.0f), M2 = mk3(0.0f, 0.0f, 0.0f);
	float count = 0.0f;
#pragma unroll
	for (int dy = -3; dy <= 3; ++dy) {
		const int32_t qy = (int32_t) py + dy;
		if ((uint32_t) qy >= f.height) continue;
		const size_t row = (size_t) qy * f.width;
		float4 tap_position[7], tap_normal[7], tap_colour[7], tap_moments[7];
		bool inside[7];
#pragma unroll
		for (int dx = -3; dx <= 3; ++dx) {
			const int32_t qx = (int32_t) px + dx;
			inside[dx + 3] = (uint32_t) qx < f.width;
			const size_t q = row + (size_t) (inside[dx + 3] ? qx : (int32_t) px);
			tap_position[dx + 3] = f.position[q];
			tap_normal[dx + 3] = f.normal[q];
			tap_colour[dx + 3] = f.new_colour[q];
			tap_moments[dx + 3] = f.new_moments[q];
		}
#pragma unroll
		for (int dx = -3; dx <= 3; ++dx) {
			const int i = dx + 3;
			if (dx != 0 || dy != 0) {
				if (!inside[i] || !(tap_position[i].w > 0.0f) || !(tap_colour[i].w > 0.0f)) continue;
				if (!same_surface(f, P_p, n_p, d_z, rgb(tap_position[i]), rgb(tap_normal[i]))) continue;
			}
			count = count + 1.0f;
			M1 = M1 + rgb(tap_colour[i]);
			M2 = M2 + rgb(tap_moments[i]);
		}
	}
	M1 = divide3_full_range(M1, count);
	M2 = divide3_full_range(M2, count);
	f3 v = gmax3(0.0f, M2 - M1 * M1) * divide_full_range(1.0f, n_p_length);
	if (f.modulation) {
		const f3 m = modulation_of(f.modulation[p]);
		v = v * (m * m);
	}
	f.out_variance[p] = make_float4(v.x, v.y, v.z, 1.0f);
}

// ---- host side ---------------------------------------------------------------------------------------------------

// The two sets of colour, moments, position and normal, and the event behind the last call
static frame_image_set images_of(frame_history_t* history) {
	return {"history", &history->width, &history->height, &history->accumulated, 8,
		{&history->colour[0], &history->colour[1], &history->moments[0], &history->moments[1], &history->position[0], &history->position[1], &history->normal[0], &history->normal[1]}};
}

extern "C" void destroy_frame_history(frame_history_t* history, application_t* app) {
	destroy_frame_images(images_of(history), app);
	memset(history, 0, sizeof(*history));
}

extern "C" int create_frame_history(frame_history_t* history, application_t* app, uint32_t width, uint32_t height) {
	memset(history, 0, sizeof(*history));
	// (cleared: reset_frame_history() touches no memory, and no call reads a set before one wrote it, but read() may)
	return create_frame_images(images_of(history), app, width, height, VKR_FRAME_HISTORY_MAX_EXTENT, true, "images");
}

extern "C" void reset_frame_history(frame_history_t* history) {
	if (history) history->frame_count = 0;
}

// Both entry points; `function`: the caller's name, for messages
static int accumulate(const char* function, frame_history_t* history, application_t* app, const frame_history_settings_t* settings, const frame_history_images_t* images, const void* previous_position) {
	if (!history || !app || !settings || !images) {
		printf("%s() needs a history, an application, settings and images.\n", function);
		return 1;
	}
	// (written so that a NaN fails)
	if (!(settings->max_length >= 1.0f && settings->max_length < INFINITY) || !(settings->sigma_depth > 0.0f && settings->sigma_depth < INFINITY)
		|| !(settings->normal_threshold >= -1.0f && settings->normal_threshold <= 1.0f) || settings->spatial_length > VKR_FRAME_HISTORY_MAX_SPATIAL_LENGTH)
	{
		printf("%s() takes a finite largest length >= 1, a finite sigma of the depth > 0, a normal threshold from -1 to 1 and a spatial length up to %d.\n", function, VKR_FRAME_HISTORY_MAX_SPATIAL_LENGTH);
		return 1;
	}
	const frame_call call = {function, {images->colour, images->position, images->normal, images->reprojection, images->modulation, previous_position}, {images->out_colour, images->out_variance}};
	if (check_frame_call_images(call, images->colour && images->position && images->normal && images->out_colour)) return 1;
	const frame_image_set own = images_of(history);
	if (!frame_images_created(own) || history->current >= 2) {
		printf("%s() needs a history created by create_frame_history().\n", function);
		return 1;
	}
	const size_t bytes = frame_image_bytes(own);
	hipStream_t stream;
	if (check_frame_call_overlap(call, bytes, &own) || begin_frame_call(call, app, bytes, &stream)) return 1;
	const uint32_t old_set = history->current, new_set = old_set ^ 1u;
	history_frame f;
	f.colour = (const float4*) images->colour;
	f.position = (const float4*) images->position;
	f.normal = (const float4*) images->normal;
	f.reprojection = (const float4*) images->reprojection;
	f.modulation = (const float4*) images->modulation;
	f.previous_position = (const float4*) previous_position;
	f.old_colour = (const float4*) history->colour[old_set];
	f.old_moments = (const float4*) history->moments[old_set];
	f.old_position = (const float4*) history->position[old_set];
	f.old_normal = (const float4*) history->normal[old_set];
	f.new_colour = (float4*) history->colour[new_set];
	f.new_moments = (float4*) history->moments[new_set];
	f.new_position = (float4*) history->position[new_set];
	f.new_normal = (float4*) history->normal[new_set];
	f.out_colour = (float4*) images->out_colour;
	f.out_variance = (float4*) images->out_variance;
	f.width = history->width;
	f.height = history->height;
	f.has_history = history->frame_count != 0;
	f.max_length = settings->max_length;
	f.sigma_depth = settings->sigma_depth;
	f.normal_threshold = settings->normal_threshold;
	f.spatial_length = (float) settings->spatial_length;
	dim3 grid((f.width + 15) / 16, (f.height + 15) / 16);
	if (previous_position) {
		if (images->out_variance) k_accumulate_history<true, true><<<grid, 256, 0, stream>>>(f);
		else k_accumulate_history<false, true><<<grid, 256, 0, stream>>>(f);
	}
	else if (images->out_variance) k_accumulate_history<true, false><<<grid, 256, 0, stream>>>(f);
	else k_accumulate_history<false, false><<<grid, 256, 0, stream>>>(f);
	if (hip_failed(hipGetLastError(), "accumulating a frame")) return 1;
	if (images->out_variance && settings->spatial_length) {
		k_history_spatial_variance<<<grid, 256, 0, stream>>>(f);
		if (hip_failed(hipGetLastError(), "estimating the variance of short histories")) return 1;
	}
	history->current = new_set;
	// (a counter that wrapped to 0 would drop the history)
	if (history->frame_count != UINT32_MAX) ++history->frame_count;
	return finish_frame_call(call, app, bytes, history->accumulated, "marking the accumulated frame");
}

extern "C" int accumulate_frame_history(frame_history_t* history, application_t* app, const frame_history_settings_t* settings, const frame_history_images_t* images) {
	return accumulate("accumulate_frame_history", history, app, settings, images, NULL);
}

extern "C" int accumulate_moving_frame_history(frame_history_t* history, application_t* app, const frame_history_settings_t* settings, const frame_history_images_t* images, const void* previous_position) {
	return accumulate("accumulate_moving_frame_history", history, app, settings, images, previous_position);
}
