/* Frame filter: an edge-avoiding a-trous wavelet on the device (Dammertz et al. 2010) with the variance-guided luminance
 * weight of SVGF (Schied et al. 2017).  One call filters an image the caller names, guided by images the caller names:
 * the mean and variance of resolve_frame_statistics(), position and normal of render_feature_buffers(), the diffuse albedo
 * as modulation.  No history, no state besides scratch images.  No reference counterpart.
 *
 * All arithmetic is IEEE binary32 with every operation rounded on its own (nothing contracted, denormals kept), in an order
 * that is part of the interface: vulkan_renderer_amd/frame_filter.py restates it in numpy, bit for bit.  a / b and sqrt are
 * the correctly rounded ones over the whole exponent range (variances and weights leave the windows of the short chains of
 * csrc/device_math.h); dot(), gmax() and exp2_poly() are those of csrc/device_math.h:
 *     dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z,   gmax(x, y) = x < y ? y : x
 *     lum(r, g, b) = (0.2126f * r + 0.7152f * g) + 0.0722f * b
 * Pixel p = (x, y) has index y * width + x.  Sums start from +0.
 *
 * Covered.  A pixel is covered if position.w > 0 (a NaN is not): position.w is the distance of pixel_feature_position, 0
 * where nothing is visible.  An uncovered p gets the sixteen bytes of colour[p], and of variance[p], unchanged; an uncovered
 * q is never a tap.
 *
 * Prepare.  m_c = gmax(modulation_c, 1 / 256) per channel (m = 1 without a modulation image);
 *     c0 = colour / m,   v0 = (variance * variance_scale) / (m * m)
 *
 * Iteration i = 0 ... n - 1 with step s = 2^i, at a covered p:
 *     l_p = lum(c_p)
 *     vbar = sum(g * v_q) / sum(g) per channel over the in-frame covered q of the 3x3 pixels around p at distance 1
 *         (not dilated), in row-major order, g = 1/4 for p, 1/8 for its four neighbours, 1/16 for the diagonal ones
 *     d_l = sigma_luminance * lum(sqrt(vbar.r), sqrt(vbar.g), sqrt(vbar.b)) + 1e-8f
 *         (the channels of one pixel share their samples: they are treated as fully correlated, so the standard deviation
 *         of the luminance is the luminance of the standard deviations)
 *     d_z = sigma_depth * position_p.w
 *     for dy = -2 ... 2, for dx = -2 ... 2:  q = p + s * (dx, dy); skipped when out of the frame or not covered
 *         h = K[|dx|] * K[|dy|], K = {3/8, 1/4, 1/16} (exact)
 *         the centre tap: w = h, whatever its guides say (sum_w >= 9/64)
 *         every other tap:
 *             w_n = gmax(0, dot(n_p, n_q)), then w_n = w_n * w_n, normal_squarings times
 *             e_z = |dot(n_p, P_q - P_p)| / d_z
 *             e_l = |l_q - l_p| / d_l, l_q = lum(c_q); 0 without a variance image
 *             t = -(e_z + e_l) * 1.44269502f
 *             w_e = exp2_poly(t) if t >= -126, else 0 (a NaN gives 0)
 *             w = (h * w_n) * w_e; a tap whose w is not > 0 is skipped: a NaN or infinite pixel does not cross an edge
 *         sum_c += w * c_q,  sum_v += (w * w) * v_q,  sum_w += w   (per channel; product and sum are separate operations)
 *     c' = sum_c / sum_w,  v' = sum_v / (sum_w * sum_w);  alpha of c' is that of c_p
 *
 * Finish.  out_colour.rgb = c_n * m, out_colour.a = the bits of colour[p].a; out_variance.rgb = v_n * (m * m), alpha 1.
 *
 * One kernel launch per iteration; prepare is part of the first and finish of the last. */
#ifndef VKR_FRAME_FILTER_H
#define VKR_FRAME_FILTER_H
#include "vkr_shading_pass.h"

#define VKR_FRAME_FILTER_MAX_ITERATIONS 5
#define VKR_FRAME_FILTER_MAX_NORMAL_SQUARINGS 8
/*! largest width and height of a filter */
#define VKR_FRAME_FILTER_MAX_EXTENT 32768

typedef struct frame_filter_settings_s {
	uint32_t iteration_count;   /* 1 ... 5; iteration i uses step 2^i */
	uint32_t normal_squarings;  /* 0 ... 8; the cosine is squared this many times (7: power 128) */
	float sigma_luminance;      /* finite, > 0 */
	float sigma_depth;          /* finite, > 0: plane distance in units of the distance to the camera */
	float variance_scale;       /* finite, >= 0: e.g. 1 / n when `variance` is the variance of ONE frame and `colour` the mean of n */
} frame_filter_settings_t;

/*! device pointers to width * height pixels of 16 bytes, row-major, 16-byte aligned */
typedef struct frame_filter_images_s {
	const void* colour;      /* RGBA32F, required */
	const void* variance;    /* RGBA32F, may be NULL: no luminance weight, no variance output */
	const void* position;    /* pixel_feature_position, required */
	const void* normal;      /* pixel_feature_normal, required */
	const void* modulation;  /* RGBA32F, may be NULL: e.g. pixel_feature_diffuse_albedo; colour is divided by it before and multiplied after */
	void* out_colour;        /* RGBA32F, required */
	void* out_variance;      /* RGBA32F, may be NULL; refused without `variance` */
} frame_filter_images_t;

typedef struct frame_filter_s {
	uint32_t width, height;
	/*! device memory, width * height * 16 bytes each: what iteration i writes and iteration i + 1 reads */
	void* colour_scratch[2];
	void* variance_scratch[2];
	/*! hipEvent_t: the end of the most recent filter_frame() */
	void* filtered;
} frame_filter_t;

/*! width = height = 0: app->swapchain.extent.  Returns 0 on success, 1 on failure (message printed). */
VKR_API int create_frame_filter(frame_filter_t* filter, application_t* app, uint32_t width, uint32_t height);
/*! Waits for app->device.stream and frees everything */
VKR_API void destroy_frame_filter(frame_filter_t* filter, application_t* app);
/*! Queues settings->iteration_count kernels on app->device.stream and returns at once.  Needs no shading pass and no scene.
	Any device buffers of the filter's extent; where one is a target of the pass, the call behaves like accumulate_frames()
	and resolve_frame_statistics(): it goes behind the frames in flight, and a later frame that writes an input or an output
	waits for the filter on the device, in front of the kernel that does the writing.  Returns 0 on success; 1 after printing
	one line, with nothing written, for a filter that was not created, a missing or misaligned image, an output that
	overlaps an input or the other output, out_variance without variance and settings outside their ranges (a NaN fails). */
VKR_API int filter_frame(frame_filter_t* filter, application_t* app, const frame_filter_settings_t* settings, const frame_filter_images_t* images);

#endif
