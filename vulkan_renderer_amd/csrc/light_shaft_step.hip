// The light shaft step of a band: which patches need no shadow rays toward which lights, the verdicts that are kept while
// their inputs stand still, and the diagnostics that read the shaft tables (light_shafts.h defines non-template kernels:
// this unit alone may include it).
#include "light_shafts.h"
#include "frame_pipeline.h"

using namespace vkr;

void create_light_shafts(frame_pipeline* frames) {
	frames->light_shafts = environment_knob("VKR_LIGHT_SHAFTS", 2u, 0u, 2u);
	// VKR_SHAFT_LISTS=0: a shaft walk ends at the first triangle in the way (no occluder lists, light_shafts.h)
	frames->shaft_lists = environment_knob("VKR_SHAFT_LISTS", 1u, 0u, 1u);
	// VKR_SHAFT_REST: frames (of a frame context) for which a pair is not walked again after a walk that met more triangles
	// than a list holds; 0: every pair is walked in every frame (light_shafts.h, kShaftResting)
	frames->shaft_rest = environment_knob("VKR_SHAFT_REST", kShaftRestFrames, 0u, 200u);
	// VKR_SHAFT_MAX_STEPS: steps after which a walk gives up (plus a fifth of it per light that is walked along).  The shaft
	// kernel of a small launch - a rank's slab at N = 8 - lasts as long as its longest walk.
	// (0: by the size of the launch - kShaftMaxSteps, or kShaftSmallLaunchSteps below 12 288 shading waves)
	frames->shaft_max_steps = environment_knob("VKR_SHAFT_MAX_STEPS", 0u, 0u, 1000u);
}

void destroy_light_shafts(wavefront_buffers* w) {
	(void) hipFree(w->shaft_clear);
	(void) hipFree(w->shaft_rectangles);
	(void) hipFree(w->shaft_lists);
	free_inputs(&w->shaft_seen);
}

// the techniques whose samples aim at the light polygon itself: every shadow ray lies inside the light's shaft
static bool aims_at_light_polygon(int technique) {
	return technique == kTechniquePsa || technique == kTechniquePsaBiased || technique == kTechniqueSolidAngle || technique == kTechniqueClippedSolidAngle;
}

// light shafts: which patches need no shadow rays toward which lights (light_shafts.h).  For the techniques
// whose samples aim at the light polygon itself (every ray then lies inside the shaft); the walk uses the
// four-wide tree whatever tree the rays walk.
static bool light_shafts_apply(const application_t* app, const frame_plan* f, const frame_context* frame) {
	const frame_pipeline* frames = f->frames;
	const uint32_t rays_per_pixel = app->render_settings.sample_count * f->p.light_count * (f->strategy == (int) sampling_strategies_diffuse_only ? 1u : 2u);
	return frame && (frames->light_shafts == 1u || (frames->light_shafts == 2u && rays_per_pixel >= 8u)) && is_deferred(f->ray_mode) && f->error_mode == kErrorNone
		&& app->scene.acceleration_structure.wide_nodes && f->p.light_count
		&& app->scene.acceleration_structure.node_count < (1u << kShaftLightShift)  // (a queue entry of the walk is a node or triangle index and a light)
		&& aims_at_light_polygon(f->technique);
}

static int ensure_shaft_words(wavefront_buffers* w, size_t words, uint32_t light_count, bool lists, hipStream_t stream) {
	size_t list_words = lists ? words * kShaftListMax * kShaftListEntry : 0;
	const bool fresh_words = words > w->shaft_words;
	// (the tables carry state from frame to frame: whichever of them is allocated anew, the copy of the inputs is forgotten)
	if (list_words > w->shaft_list_words || light_count > w->shaft_rectangle_count || fresh_words) forget_inputs(&w->shaft_seen);
	if (grow_device_buffer(&w->shaft_lists, &w->shaft_list_words, list_words, sizeof(float), "Failed to allocate %.1f MiB for the occluder lists of the light shafts.\n")
		|| grow_device_buffer(&w->shaft_rectangles, &w->shaft_rectangle_count, light_count, sizeof(float4), "Failed to allocate the rectangles of the light shafts.\n")
		|| grow_device_buffer(&w->shaft_clear, &w->shaft_words, words, sizeof(uint32_t), "Failed to allocate %.1f MiB for the light shafts.\n"))
		return 1;
	// (the shaft kernel reads the verdicts of the frame before: none yet)
	if (fresh_words && hipMemsetAsync(w->shaft_clear, 0, words * sizeof(uint32_t), stream) != hipSuccess) {
		w->shaft_words = 0;
		return 1;
	}
	return 0;
}

// What the verdicts of a launch are derived from, as bytes (light_shafts.h "Verdicts that are still true"): a frame context
// keeps the image of its most recent launch (wavefront_buffers::shaft_seen) and the next launch is compared with it -
// "the same" now keeps a "clear" or a list.
// The image has two parts.  The ARRANGEMENT is this struct and, behind it, the ranges of the constants that the shading
// positions are computed from (the camera's, the mesh's de-quantisation); then comes one record per LIGHT, its bytes in
// the constants.
// Camera, lights and the de-quantisation reach the kernels through write_constants() alone, whose bytes are compared
// themselves; everything else: launch_inputs (frame_pipeline.h).
struct shaft_arrangement {
	launch_inputs head;
	uint32_t lists, groups, max_steps, build_bits, node_count, wide_node_count;
	float extent;
	uint32_t light_stride;
	const void *nodes, *triangles, *wide_nodes;
	float grid_origin[3], grid_inverse_cell[3];
};
static_assert(sizeof(shaft_arrangement) == sizeof(launch_inputs) + 8 * 4 + 3 * sizeof(void*) + 6 * 4, "no padding: the struct is compared as bytes");

// Puts the image of this launch's inputs together, compares it with the context's copy and keeps it as the new copy.
// -> arrangement_same, same_lights (bit i: arrangement and light i < 32 are byte-equal to the previous launch's)
static int compare_shaft_inputs(frame_pipeline* frames, wavefront_buffers* w, const shading_pass_t* pass, const shaft_arrangement& arrangement, bool& arrangement_same, uint32_t& same_lights) {
	arrangement_same = false;
	same_lights = 0u;
	const uint8_t* constants = (const uint8_t*) pass->constants_host;
	const size_t ranges[2][2] = {{offsetof(per_frame_constants_t, world_to_projection_space), offsetof(per_frame_constants_t, mis_visibility_estimate)},
		{offsetof(per_frame_constants_t, mesh_dequantization_factor), offsetof(per_frame_constants_t, error_factor)}};
	const uint32_t light_count = arrangement.head.light_count;
	const size_t light_bytes = (size_t) arrangement.light_stride * light_count;
	size_t arrangement_bytes = sizeof(shaft_arrangement);
	for (const size_t* range : ranges) arrangement_bytes += range[1] - range[0];
	const size_t size = arrangement_bytes + light_bytes;
	uint8_t* now = begin_inputs(&w->shaft_seen, &frames->scratch, size);
	if (!now) {
		printf("Failed to allocate %zu bytes for the inputs of the light shafts.\n", size);
		return 1;
	}
	memcpy(now, &arrangement, sizeof(arrangement));
	size_t cursor = sizeof(arrangement);
	for (const size_t* range : ranges) {
		memcpy(now + cursor, constants + range[0], range[1] - range[0]);
		cursor += range[1] - range[0];
	}
	memcpy(now + cursor, constants + sizeof(per_frame_constants_t), light_bytes);
	if (same_inputs(&w->shaft_seen, now, size, 0, arrangement_bytes)) {
		arrangement_same = true;
		for (uint32_t i = 0; i != light_count && i != 32u; ++i)
			if (same_inputs(&w->shaft_seen, now, size, arrangement_bytes + (size_t) arrangement.light_stride * i, arrangement.light_stride)) same_lights |= 1u << i;
	}
	keep_inputs(&w->shaft_seen, now, size);
	return 0;
}

int run_light_shafts(application_t* app, frame_plan* f, frame_context* frame, hipStream_t stream) {
	shading_pass_t* pass = &app->shading_pass;
	shade_params& p = f->p;
	p.shaft_clear = NULL;
	p.shaft_rectangles = NULL;
	p.shaft_lists = NULL;
	if (!light_shafts_apply(app, f, frame)) {
		pass->last_shaft_groups = 0;
		return 0;
	}
	frame_pipeline* frames = f->frames;
	const acceleration_structure_t* structure = &app->scene.acceleration_structure;
	uint32_t shaft_groups = shade_grid_size(p.block_count);
	const bool lists = frames->shaft_lists != 0u && kShaftListMax != 0u;
	if (ensure_shaft_words(&frame->buffers, (size_t) shaft_groups * p.light_count + 8, p.light_count, lists, stream)) return 1;
	float extent = 0.0f;
	for (int j = 0; j != 3; ++j) extent = fmaxf(extent, kGridMax / structure->grid_inverse_cell[j]);
	// (VKR_SHAFT_COUNTERS=1: the walks count their steps into three words behind the table, for get_light_shaft_work())
	static const bool count_work = getenv("VKR_SHAFT_COUNTERS") != NULL;
	unsigned long long* work = NULL;
	if (count_work) {
		work = (unsigned long long*) (frame->buffers.shaft_clear + (((size_t) shaft_groups * p.light_count + 1u) & ~(size_t) 1u));
		(void) hipMemsetAsync(work, 0, 3 * sizeof(unsigned long long), stream);
	}
	// (a small launch lasts as long as its longest walk: plan_bands(), at trace_blocks)
	const uint32_t max_steps = frames->shaft_max_steps ? frames->shaft_max_steps : (shaft_groups < 12288u ? kShaftSmallLaunchSteps : kShaftMaxSteps);
	shaft_arrangement arrangement;
	memset(&arrangement, 0, sizeof(arrangement));
	fill_launch_inputs(arrangement.head, p, frames, structure);
	arrangement.lists = lists ? 1u : 0u; arrangement.groups = shaft_groups; arrangement.max_steps = max_steps;
	memcpy(&arrangement.build_bits, &structure->build_milliseconds, sizeof(arrangement.build_bits));
	arrangement.node_count = structure->node_count; arrangement.wide_node_count = structure->wide_node_count;
	arrangement.extent = extent;
	arrangement.light_stride = (uint32_t) ((pass->constants_size - sizeof(per_frame_constants_t)) / p.light_count);
	arrangement.nodes = p.bvh.nodes; arrangement.triangles = p.bvh.triangles; arrangement.wide_nodes = structure->wide_nodes;
	for (int j = 0; j != 3; ++j) {
		arrangement.grid_origin[j] = structure->grid_origin[j];
		arrangement.grid_inverse_cell[j] = structure->grid_inverse_cell[j];
	}
	bool arrangement_same;
	uint32_t same_lights;
	if (compare_shaft_inputs(frames, &frame->buffers, pass, arrangement, arrangement_same, same_lights)) return 1;
	// VKR_SHAFT_REST=0, "every pair is walked in every frame": nothing rests and nothing is kept
	if (frames->shaft_rest == 0u) { arrangement_same = false; same_lights = 0u; }
	// (The kernel is launched even when the host expects every verdict to be kept: which pairs still rest, and which walks are
	// due again, only the table on the device knows.  A launch whose waves read their words and leave: DESIGN.md 4.3.)
	k_light_shafts<<<shaft_groups, 64, 0, stream>>>(p, (const uint4*) structure->wide_nodes, frame->buffers.shaft_clear, frame->buffers.shaft_rectangles, lists ? frame->buffers.shaft_lists : NULL, extent, work,
		arrangement_same ? 1u : 0u, same_lights, frames->shaft_rest, max_steps);
	if (hip_failed(hipGetLastError(), "launching the light shaft kernel")) {
		// (what the tables hold now is anybody's guess)
		forget_inputs(&frame->buffers.shaft_seen);
		return 1;
	}
	p.shaft_clear = frame->buffers.shaft_clear;
	p.shaft_rectangles = frame->buffers.shaft_rectangles;
	p.shaft_lists = lists ? frame->buffers.shaft_lists : NULL;
	pass->last_shaft_groups = shaft_groups;
	return 0;
}

// sums the words of the most recent launch's shaft table
// out[0]: clear pairs, out[1 ... 5]: pairs that are traced, by reason (kShaftNoPixels ... kShaftTriangle, light_shafts.h),
// out[6]: anything else, out[7]: pairs with an occluder list, out[8]: triangles on those lists
__global__ void __launch_bounds__(256) k_count_clear_shafts(const uint32_t* words, size_t count, unsigned long long* out) {
	for (size_t i = (size_t) blockIdx.x * 256u + threadIdx.x; i < count; i += (size_t) gridDim.x * 256u) {
		uint32_t verdict = words[i] & 0xFFu;
		uint32_t slot = verdict == kShaftClear ? 0u : (verdict == kShaftList ? 7u : (verdict >= kShaftNoPixels && verdict <= kShaftTriangle ? 1u + (verdict - kShaftNoPixels) : 6u));
		atomicAdd(out + slot, 1ull);
		if (verdict == kShaftList) atomicAdd(out + 8, (unsigned long long) ((words[i] >> 8) & 0x1Fu));
	}
}

extern "C" int get_light_shaft_statistics(application_t* app, uint64_t out_statistics[12]) {
	memset(out_statistics, 0, sizeof(uint64_t) * 12);
	const shading_pass_t* pass = &app->shading_pass;
	const wavefront_buffers* w = last_launch_buffers(app);
	if (!w || !pass->last_shaft_groups || !w->shaft_clear) return 0;  // the last frame ran without the shaft test: all zero
	if (finish_frames(app)) return 1;
	size_t words = (size_t) pass->last_shaft_groups * app->scene_specification.polygonal_light_count;
	unsigned long long* counter = NULL;
	if (hip_failed(hipMalloc(&counter, sizeof(unsigned long long) * 16), "allocating counters")) return 1;
	hipStream_t stream = (hipStream_t) app->device.stream;
	(void) hipMemsetAsync(counter, 0, sizeof(unsigned long long) * 16, stream);
	k_count_clear_shafts<<<256, 256, 0, stream>>>(w->shaft_clear, words, counter);
	unsigned long long counts[16] = {0};
	int failed = vkr_copy_to_host(counts, counter, sizeof(counts), &app->device);
	(void) hipFree(counter);
	out_statistics[0] = words;
	out_statistics[1] = counts[0];
	out_statistics[2] = pass->last_shaft_groups;
	out_statistics[3] = app->scene_specification.polygonal_light_count;
	for (int i = 0; i != 6; ++i) out_statistics[4 + i] = counts[1 + i];
	out_statistics[10] = counts[7];
	out_statistics[11] = counts[8];
	return failed;
}

// (diagnostics, VKR_SHAFT_COUNTERS=1) {steps, triangle batches, walks} of the most recent launch's shaft kernel
extern "C" int get_light_shaft_work(application_t* app, uint64_t out_work[3]) {
	out_work[0] = out_work[1] = out_work[2] = 0;
	const shading_pass_t* pass = &app->shading_pass;
	const wavefront_buffers* w = last_launch_buffers(app);
	if (!w || !pass->last_shaft_groups || !w->shaft_clear || !getenv("VKR_SHAFT_COUNTERS") || finish_frames(app)) return 0;
	size_t words = ((size_t) pass->last_shaft_groups * app->scene_specification.polygonal_light_count + 1u) & ~(size_t) 1u;
	return vkr_copy_to_host(out_work, w->shaft_clear + words, 3 * sizeof(uint64_t), &app->device);
}

// (diagnostics) the verdict words of the most recent launch, [patch][light]; returns how many were written
extern "C" uint64_t read_back_light_shafts(application_t* app, uint32_t* out_words, uint64_t capacity) {
	const shading_pass_t* pass = &app->shading_pass;
	const wavefront_buffers* w = last_launch_buffers(app);
	if (!w || !pass->last_shaft_groups || !w->shaft_clear || finish_frames(app)) return 0;
	uint64_t words = (uint64_t) pass->last_shaft_groups * app->scene_specification.polygonal_light_count;
	if (words > capacity) words = capacity;
	if (vkr_copy_to_host(out_words, w->shaft_clear, sizeof(uint32_t) * words, &app->device)) return 0;
	return words;
}
