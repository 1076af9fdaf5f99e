/* Frame history: temporal accumulation on the device.  One call blends the frame the caller names into a history that is
 * found where each pixel was under the previous camera (pixel_feature_reprojection of render_feature_buffers(), rendered
 * with the PREVIOUS frame's world_to_projection_space), and gives the accumulated colour and its variance: what
 * filter_frame() takes as colour and variance with variance_scale 1.  The history is two sets of four images that take
 * turns.  accumulate_frame_history() sees the camera only; accumulate_moving_frame_history() follows geometry that
 * update_scene_geometry() moved, with the images of render_motion_buffers() (the last paragraph).  No reference counterpart.
 *
 * All arithmetic is IEEE binary32 with every operation rounded on its own (nothing contracted, denormals kept), in an order
 * that is part of the interface: vulkan_renderer_amd/frame_history.py restates it in numpy, bit for bit.  a / b is the
 * correctly rounded quotient over the whole exponent range (divide_full_range() of csrc/device_math.h); dot(), gmax() and
 * gmin() are those of csrc/device_math.h:
 *     dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z,   gmax(x, y) = x < y ? y : x,   gmin(x, y) = y < x ? y : x
 * Pixel p = (x, y) has index y * width + x.  Sums start from +0.  x * y + z is a product and a sum.  Every comparison is
 * written so that a NaN fails it.  h is the set that the previous call wrote, h' the one that this call writes.
 *
 * Covered.  A pixel is covered if position.w > 0, as in the frame filter.  An uncovered p gets sixteen zero bytes in
 * h'.colour, h'.moments and out_variance, the sixteen bytes of position[p] and normal[p] in h'.position and h'.normal, and
 * the sixteen bytes of colour[p] in out_colour.  The rest is about a covered p.
 *
 * Prepare.  m_c = gmax(modulation_c, 1 / 256) per channel (m = 1 without a modulation image, and then neither the
 * quotient nor the products with m are computed: they change no bit of what is stored);
 *     c = colour.rgb / m,   s = c * c
 * The sample is finite if |c| < inf in every channel.  (s overflows for |c| >= 2^64: radiance is expected to stay below.)
 *
 * Where it was.  r = reprojection[p], or {x, y, 1, 1} without the image; X = r.x, Y = r.y.  Nothing of r is trusted.  The
 * pixel is usable iff frame_count > 0, r.w == 1.0f, X >= -1, X < width, Y >= -1 and Y < height.  For a pixel that is not
 * usable the rest of this paragraph and the next two are skipped (no X or Y outside these bounds is ever turned into an
 * integer).
 *     fx = floorf(X), tx = X - fx,  fy = floorf(Y), ty = Y - fy
 *     tap k = 0 ... 3 is q = (fx + (k & 1), fy + (k >> 1)) with b_k = bx * by,
 *         bx = (k & 1) ? tx : 1 - tx,   by = (k >> 1) ? ty : 1 - ty
 *
 * A tap counts iff, decided in this order,
 *     it is in the frame (checked on the integers, 0 <= q.x < width and 0 <= q.y < height, for every tap),
 *     b_k > 0,
 *     h.position[q].w > 0,
 *     |dot(n_p, P_q - P_p)| <= sigma_depth * position_p.w,      n_p = normal[p].xyz, P_p = position[p].xyz,
 *     dot(n_p, n_q) >= normal_threshold                         P_q = h.position[q].xyz, n_q = h.normal[q].xyz
 * The positions are in world space: a point that did not move differs by rounding only.
 *
 * Sums over the taps that count, in the order k = 0 ... 3:
 *     sum_b += b,  sum_c += b * h.colour[q].rgb,  sum_s += b * h.moments[q].rgb,  sum_n += b * h.colour[q].a
 *
 * History exists iff the pixel is usable and sum_b >= 1 / 64.  Then
 *     hc = sum_c / sum_b,  hs = sum_s / sum_b,  n = sum_n / sum_b
 *     a finite sample:  n' = gmin(n + 1, max_length),  a = 1 / n',  c' = hc + a * (c - hc),  s' = hs + a * (s - hs)
 *     any other sample leaves the history as it is:  c' = hc, s' = hs, n' = n
 * No history:
 *     a finite sample:  c' = c, s' = s, n' = 1
 *     any other sample: c' = s' = 0, n' = 0
 * so that a NaN or an infinite colour never enters the history.
 *
 * Stores.  h'.colour = {c', n'},  h'.moments = {s', 0},  h'.position and h'.normal get the bytes of position[p], normal[p];
 *     out_colour = {c' * m, the bits of colour[p].a}
 *     v = gmax(0, s' - c' * c') * (1 / gmax(n', 1)) per channel,   out_variance = {v * (m * m), 1}
 * (the variance of the mean of n' samples, from the variance of one)
 *
 * Spatial variance: a second launch, only with out_variance and spatial_length > 0, for every covered p with
 * 0 < n' < (float) spatial_length - a history too short for its own second moment to say much.  It visits the 7x7 pixels
 * q = p + (dx, dy), dy = -3 ... 3 outside, dx = -3 ... 3 inside, the centre in its place.  The centre always counts; any
 * other q counts iff it is in the frame, position[q].w > 0, h'.colour[q].a > 0, |dot(n_p, P_q - P_p)| <= sigma_depth *
 * position_p.w and dot(n_p, n_q) >= normal_threshold, P_q and n_q from this frame's position and normal.
 *     k += 1,  M1 += h'.colour[q].rgb,  M2 += h'.moments[q].rgb;   then M1 = M1 / k,  M2 = M2 / k
 *     v = gmax(0, M2 - M1 * M1) * (1 / n'_p),   out_variance[p] = {v * (m * m), 1}
 * Every other pixel keeps what the first launch wrote.
 *
 * Then current ^= 1 and frame_count += 1.
 *
 * Moving geometry.  accumulate_moving_frame_history() takes reprojection from render_motion_buffers()
 * (include/vkr_motion_buffers.h), which looks the pixel's surface up where it was, and that call's previous_position
 * image.  The rule above has one change: in the tap test of "A tap counts iff", P_p = previous_position[p].xyz - the
 * point whose history the tap holds, in the world space of the frame that stored it, so that a surface that moved by more
 * than sigma_depth * position_p.w along its normal still finds its history.  n_p and the scale position_p.w stay this
 * frame's: the normals of the previous frame are not kept, and a rotation of one frame's worth is what normal_threshold and
 * sigma_depth already have to tolerate.  The stores (h'.position gets position[p]), the spatial variance launch, coverage,
 * the order of the checks and every refusal are unchanged. */
#ifndef VKR_FRAME_HISTORY_H
#define VKR_FRAME_HISTORY_H
#include "vkr_frame_filter.h"

#define VKR_FRAME_HISTORY_MAX_SPATIAL_LENGTH 64
/*! largest width and height of a history: that of the frame filter */
#define VKR_FRAME_HISTORY_MAX_EXTENT VKR_FRAME_FILTER_MAX_EXTENT

typedef struct frame_history_settings_s {
	float max_length;        /* finite, >= 1: the history length saturates here (1: nothing is accumulated) */
	float sigma_depth;       /* finite, > 0: plane distance in units of the distance to the camera, as in the filter */
	float normal_threshold;  /* finite, -1 ... 1: smallest cosine between this frame's normal and the history's */
	uint32_t spatial_length; /* 0 ... 64: pixels whose length is below it get the spatial variance estimate; 0: none do */
} frame_history_settings_t;

/*! device pointers to width * height pixels of 16 bytes, row-major, 16-byte aligned */
typedef struct frame_history_images_s {
	const void* colour;        /* RGBA32F, required: this frame */
	const void* position;      /* pixel_feature_position of this frame, required */
	const void* normal;        /* pixel_feature_normal of this frame, required */
	const void* reprojection;  /* pixel_feature_reprojection under the PREVIOUS frame's matrix; NULL: every pixel stays where it is */
	const void* modulation;    /* may be NULL; as in filter_frame() */
	void* out_colour;          /* RGBA32F, required: the accumulated colour */
	void* out_variance;        /* RGBA32F, may be NULL: the variance of out_colour, what filter_frame() takes with variance_scale 1 */
} frame_history_images_t;

/*! device memory, width * height * 16 bytes per image; set `current` is h of the next call */
typedef struct frame_history_s {
	uint32_t width, height;
	void* colour[2];    /* c' demodulated, alpha = length n' */
	void* moments[2];   /* s' = mean of c * c, alpha 0 */
	void* position[2];  /* the sixteen bytes of the frame's position */
	void* normal[2];    /* the sixteen bytes of the frame's normal */
	uint32_t current;     /* the set that holds the last accumulated frame */
	uint32_t frame_count; /* 0: no history */
	void* accumulated;    /* hipEvent_t */
} frame_history_t;

/*! width = height = 0: app->swapchain.extent.  Returns 0 on success, 1 on failure (message printed). */
VKR_API int create_frame_history(frame_history_t* history, application_t* app, uint32_t width, uint32_t height);
/*! Waits for app->device.stream and frees everything */
VKR_API void destroy_frame_history(frame_history_t* history, application_t* app);
/*! frame_count = 0: the next frame finds no history.  Touches no memory. */
VKR_API void reset_frame_history(frame_history_t* history);
/*! Queues one kernel, or two (see above), on app->device.stream and returns at once.  Needs no shading pass and no scene.
	Any device buffers of the history's extent; where one is a target of the pass, the call behaves like filter_frame(): it
	goes behind the frames in flight, and a later frame that writes an input or an output waits for the call on the device,
	in front of the kernel that does the writing.  Returns 0 on success; 1 after printing one line, with nothing written
	and the history as it was, for a missing or misaligned image, settings outside their ranges (a NaN fails), a history
	that was not created, and an output that overlaps an input, the other output or an image of the history. */
VKR_API int accumulate_frame_history(frame_history_t* history, application_t* app, const frame_history_settings_t* settings, const frame_history_images_t* images);
/*! accumulate_frame_history() for geometry that moved ("Moving geometry" above).  previous_position: device, the
	previous_position image of render_motion_buffers() for this frame, width * height pixels of 16 bytes, 16-byte aligned;
	it is one more input: no output may overlap it, and the call is noted as its reader.  NULL: accumulate_frame_history(),
	in every byte. */
VKR_API int accumulate_moving_frame_history(frame_history_t* history, application_t* app, const frame_history_settings_t* settings, const frame_history_images_t* images,
	const void* previous_position);

#endif
