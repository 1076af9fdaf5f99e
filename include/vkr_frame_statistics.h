/* Frame statistics on the device: per-pixel sums of animated-noise frames (mean, variance) and
 * error sums of whole frames, so that estimators can be compared - RMSE against a converged image at
 * equal sample count or equal time - without reading a frame back.
 *
 * No reference counterpart: the reference leaves convergence measurements to offline tooling.
 *
 * All arithmetic is IEEE binary64 with nothing contracted, in an order that is part of the interface,
 * so that results can be restated in numpy bit for bit (vulkan_renderer_amd/frame_statistics.py).
 *
 * Accumulators.  For every pixel and each of R, G, B (alpha is ignored) two doubles; for the frames
 * x_1 ... x_n in the order they were handed over
 *     S = (...((0 + (double) x_1) + (double) x_2)...)
 *     Q = (...((0 + (double) x_1 * (double) x_1) + ...)...)
 * (the product of two floats is exact in double: only the additions round).  Non-finite samples
 * propagate by IEEE rules.
 *
 * Mean and variance, RGBA32F with alpha 1:
 *     mean = (float) (S / (double) n)
 *     v = (Q - (S * S) / (double) n) / (double) (n - 1); v < 0 becomes 0 (NaN and -0 pass through)
 *     variance = (float) v
 *
 * Error sums over pixel_count pixels, one double per R, G, B: the terms e (d * d with
 * d = (double) a - (double) b, or (double) a) are added in a fixed order.  Block B holds the pixels
 * 256 B ... 256 B + 255 in slots 0 ... 255, slots past the end hold +0.0; for s = 128, 64, ..., 1:
 * slot[j] += slot[j + s] for j < s; the block's partial is slot[0]; the total is the partials added
 * in block order, starting from +0.0. */
#ifndef VKR_FRAME_STATISTICS_H
#define VKR_FRAME_STATISTICS_H
#include "vkr_shading_pass.h"

/*! Most frames one accumulate_frames() call takes */
#define VKR_MAX_ACCUMULATED_FRAMES 8

typedef struct frame_statistics_s {
	/*! RGBA32F pixels of any dense layout that the object covers: a frame, a slab, a band */
	uint64_t pixel_count;
	/*! frames accumulated since creation or the last reset */
	uint64_t frame_count;
	/*! device memory, [channel][pixel] pairs of doubles {S, Q} (internal layout: read it with
		read_back_frame_statistics()) */
	void* sums;
	/*! hipStream_t of the object's own: its accumulations run there, in call order */
	void* stream;
	/*! hipEvent_t: marks device->stream in front of an accumulation, and the end of a resolve */
	void* source_ready;
	void* resolved;
	/*! ring of hipEvent_t, one per accumulate_frames() call in turn: the end of that call's kernel, which later
		frames that write one of its sources wait for */
	void* accumulated[VKR_MAX_ACCUMULATED_FRAMES * 2];
	uint32_t next_event;
	/*! 1 once an accumulation has been queued (`accumulated` of the previous slot is recorded) */
	uint32_t pending;
} frame_statistics_t;

/*! pixel_count 0: the frame of app->swapchain.extent.  Returns 0 on success, 1 on failure (message printed). */
VKR_API int create_frame_statistics(frame_statistics_t* stats, application_t* app, uint64_t pixel_count);
/*! Waits for the object's accumulations and frees everything */
VKR_API void destroy_frame_statistics(frame_statistics_t* stats, application_t* app);
/*! Sums and frame count back to zero, behind the accumulations queued so far */
VKR_API int reset_frame_statistics(frame_statistics_t* stats, application_t* app);
/*! Adds `count` (1 ... VKR_MAX_ACCUMULATED_FRAMES) RGBA32F device buffers of stats->pixel_count pixels, in the order
	given, with one kernel that reads and writes each accumulator once; the same bits as `count` calls with one frame
	each.  device_frames NULL: app->render_targets.radiance, once.  Returns at once: the kernel is queued on the
	object's stream behind the frames in flight (render_shading_pass() / render_and_exchange_frame()) and behind
	app->device.stream.  A later frame that WRITES one of the buffers waits for the accumulation on the device, in front
	of the kernel that does the writing (like begin_read_back()); callers that want no such wait render into a ring of
	targets. */
VKR_API int accumulate_frames(frame_statistics_t* stats, application_t* app, const void* const* device_frames, uint32_t count);
/*! Writes mean and / or variance (device RGBA32F buffers of stats->pixel_count pixels, either may be NULL) behind the
	accumulations queued so far; the results are complete for work on app->device.stream.  out_mean may be
	app->render_targets.radiance: encode_output(), take_screenshot() and read_back_*() then work on the converged image.
	A variance of fewer than two frames is refused. */
VKR_API int resolve_frame_statistics(frame_statistics_t* stats, application_t* app, void* out_mean, void* out_variance);
/*! The accumulators as host arrays [pixel][3] (either may be NULL); blocks until they have arrived */
VKR_API int read_back_frame_statistics(frame_statistics_t* stats, application_t* app, double* sums, double* squares);
/*! out[c] = sum over pixels of ((double) a - (double) b)^2 for c = R, G, B of two RGBA32F device buffers, in the order
	of additions given above; behind the frames in flight and app->device.stream; blocks until the result has arrived */
VKR_API int sum_squared_differences(application_t* app, const void* a, const void* b, uint64_t pixel_count, double out[3]);
/*! out[c] = sum over pixels of (double) a, likewise */
VKR_API int sum_frame(application_t* app, const void* a, uint64_t pixel_count, double out[3]);

#endif
