// What a caller reads about the frames it has rendered: the times between the events of the timed frames, the count of
// their rays.  (The replay kernels of get_traversal_statistics() walk with lbvh.h and have a unit of their own,
// traversal_statistics.hip; the shaft tables' diagnostics: light_shaft_step.hip.)
#include "frame_pipeline.h"

// timed frames whose events are still in the ring
static uint32_t timed_frames(const shading_pass_t* pass) { return pass->timing_cursor < pass->timing_ring_size ? pass->timing_cursor : pass->timing_ring_size; }

// slot of the i-th of the most recent `count` timed frames
static uint32_t timing_slot(const shading_pass_t* pass, uint32_t count, uint32_t i) { return (pass->timing_cursor - count + i) % pass->timing_ring_size; }

// milliseconds from `from` to `to` once `to` has completed (0 if either cannot be read)
static float elapsed_milliseconds(hipEvent_t from, hipEvent_t to) {
	float ms = 0.0f;
	if (hipEventSynchronize(to) != hipSuccess || hipEventElapsedTime(&ms, from, to) != hipSuccess) ms = 0.0f;
	return ms;
}

// the time from event `from` to event `to` of each of the most recent `count` timed frames
static uint32_t get_timed_intervals(application_t* app, uint32_t from, uint32_t to, float* out, uint32_t count) {
	const shading_pass_t* pass = &app->shading_pass;
	if (!pass->timing_ring) return 0;
	if (count > timed_frames(pass)) count = timed_frames(pass);
	for (uint32_t i = 0; i != count; ++i) {
		uint32_t slot = timing_slot(pass, count, i);
		out[i] = elapsed_milliseconds(timing_event(pass, slot, from), timing_event(pass, slot, to));
	}
	return count;
}

extern "C" uint32_t get_dispatch_milliseconds(application_t* app, float* out, uint32_t count) {
	return get_timed_intervals(app, kTimingFrameStart, kTimingFrameEnd, out, count);
}

// what a timed frame spends before its shading kernel starts: the shaft kernel (and, for textured scenes, the material resolve)
extern "C" uint32_t get_light_shaft_milliseconds(application_t* app, float* out, uint32_t count) {
	return get_timed_intervals(app, kTimingFrameStart, kTimingShadingStart, out, count);
}

extern "C" uint32_t get_shading_kernel_milliseconds(application_t* app, float* out, uint32_t count) {
	return get_timed_intervals(app, kTimingShadingStart, kTimingShadingEnd, out, count);
}

extern "C" uint32_t get_frame_period_milliseconds(application_t* app, float* out, uint32_t count) {
	shading_pass_t* pass = &app->shading_pass;
	if (!pass->timing_ring || pass->timing_cursor < 2) return 0;
	uint32_t stride = pass->timing_stride > 1 ? pass->timing_stride : 1;
	uint32_t available = timed_frames(pass) - 1;
	if (count > available) count = available;
	for (uint32_t i = 0; i != count; ++i) {
		uint32_t later = timing_slot(pass, count, i);
		uint32_t earlier = (later + pass->timing_ring_size - 1) % pass->timing_ring_size;
		out[i] = elapsed_milliseconds(timing_event(pass, earlier, kTimingFrameEnd), timing_event(pass, later, kTimingFrameEnd)) / (float) stride;
	}
	return count;
}

extern "C" float get_last_dispatch_milliseconds(application_t* app) {
	float ms = 0.0f;
	if (get_dispatch_milliseconds(app, &ms, 1) != 1) return 0.0f;
	app->shading_pass.last_dispatch_ms = ms;
	return ms;
}

extern "C" uint64_t get_last_ray_count(const application_t* app) {
	unsigned long long rays = 0;
	const shading_pass_t* pass = &app->shading_pass;
	if (!pass->ray_counter || !pass->use_ray_tracing || !pass->last_frame_traced_rays || !pass->frame_counter) return 0;
	// (the kernels of the frame - the shading kernel with inline rays, else the resolve kernel of every
	// band - added their rays to the frame's counter)
	if (finish_frames((application_t*) app)) return 0;
	if (vkr_copy_to_host(&rays, (const unsigned long long*) pass->ray_counter + (pass->frame_counter - 1u) % 16u, sizeof(rays), &app->device)) return 0;
	return rays;
}
