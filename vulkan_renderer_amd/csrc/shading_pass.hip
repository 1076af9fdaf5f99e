// The frame pipeline behind the reference's entry points (create_shading_pass src/main.c:598, write_constants :2114,
// the vkCmdDraw of record_render_frame_commands :1428-1434): variant selection, the wavefront buffers, frame plan, band
// steps (wavefront_kernels.h defines non-template kernels: this unit alone includes it, and launches them).  The band steps
// with a unit of their own, and what all of them share: frame_pipeline.h.
#include "wavefront_kernels.h"
#include "shade_launchers.h"
#include "frame_pipeline.h"

using namespace vkr;

// [arithmetic_mode_t + 3 * light textures][strategy]
#define VKR_LAUNCHER_ROW(mode) {vkr_launch_shade_##mode##_0, vkr_launch_shade_##mode##_1, vkr_launch_shade_##mode##_2, vkr_launch_shade_##mode##_3, vkr_launch_shade_##mode##_4}
static const launch_function_t g_launchers[6][5] = {
	VKR_LAUNCHER_ROW(libm), VKR_LAUNCHER_ROW(fast), VKR_LAUNCHER_ROW(exact),
	VKR_LAUNCHER_ROW(textured_libm), VKR_LAUNCHER_ROW(textured_fast), VKR_LAUNCHER_ROW(textured_exact),
};
static const error_launch_function_t g_error_launchers[3] = VKR_MODE_LAUNCHERS(vkr_launch_error_display);
static const resolve_launch_function_t g_resolve_launchers[3] = VKR_MODE_LAUNCHERS(vkr_launch_resolve_materials);

// The strategies that prepare a specular technique besides the diffuse one (the combined diffuse + specular path), and the
// out-of-range strategies, which select the same preparation (validate_settings)
static bool has_specular_technique(const render_settings_t* settings) { return settings->sampling_strategies >= sampling_strategies_diffuse_specular_separately; }

static int technique_index(const render_settings_t* settings) {
	switch (settings->polygon_sampling_technique) {
	// Arvo's sampler only exists in the diffuse-only / GGX-MIS branch of the reference shader; its
	// combined diffuse + specular branch uses the paper's own sampler whatever the technique says
	// (shading_pass.frag.glsl:441, :506-547)
	case sample_polygon_projected_solid_angle_arvo:
		return has_specular_technique(settings) ? kTechniquePsa : kTechniquePsaArvo;
	case sample_polygon_projected_solid_angle: return kTechniquePsa;
	case sample_polygon_projected_solid_angle_biased: return kTechniquePsaBiased;
	case sample_polygon_solid_angle: return kTechniqueSolidAngle;
	case sample_polygon_clipped_solid_angle: return kTechniqueClippedSolidAngle;
	case sample_polygon_baseline: return kTechniqueBaseline;
	case sample_polygon_area_turk: return kTechniqueAreaTurk;
	case sample_polygon_rectangle_solid_angle_urena: return kTechniqueUrena;
	case sample_polygon_solid_angle_arvo: return kTechniqueArvoSolidAngle;
	case sample_polygon_bilinear_cosine_warp_hart: return kTechniqueHartBilinear;
	case sample_polygon_bilinear_cosine_warp_clipping_hart: return kTechniqueHartBilinearClipping;
	case sample_polygon_biquadratic_cosine_warp_hart: return kTechniqueHartBiquadratic;
	case sample_polygon_biquadratic_cosine_warp_clipping_hart: return kTechniqueHartBiquadraticClipping;
	default: return -1;
	}
}

// the projected solid angle techniques: the only ones with an error display and with LTC importance sampling beside them
static bool is_projected_solid_angle(int technique) { return technique == kTechniquePsa || technique == kTechniquePsaBiased || technique == kTechniquePsaArvo; }

// ---- shading pass ----------------------------------------------------------------

static void free_wavefront_buffers(wavefront_buffers* w) {
	(void) hipFree(w->codes); (void) hipFree(w->terms_visible); (void) hipFree(w->terms_hidden);
	(void) hipFree(w->base_color); (void) hipFree(w->ray_directions); (void) hipFree(w->ray_records); (void) hipFree(w->ray_origins); (void) hipFree(w->ray_queue_size);
	(void) hipFree(w->spill);
	destroy_light_shafts(w);
	(void) hipFree(w->psa_table_memory);
	memset(w, 0, sizeof(*w));
}

static void destroy_wavefront(shading_pass_t* pass) {
	frame_pipeline* frames = (frame_pipeline*) pass->wavefront;
	if (!frames) return;
	for (frame_context& c : frames->contexts) {
		if (c.done) { (void) hipEventSynchronize(c.done); (void) hipEventDestroy(c.done); }
		free_wavefront_buffers(&c.buffers);
	}
	free_wavefront_buffers(&frames->device_stream_buffers);
	if (frames->inputs_ready) (void) hipEventDestroy(frames->inputs_ready);
	if (frames->readers_done) (void) hipEventDestroy(frames->readers_done);
	free(frames->scratch.bytes);
	destroy_prepared_polygons(frames);
	free(frames);
	pass->wavefront = NULL;
}

static frame_pipeline* ensure_frames(shading_pass_t* pass) {
	frame_pipeline* frames = (frame_pipeline*) pass->wavefront;
	if (frames) return frames;
	frames = (frame_pipeline*) calloc(1, sizeof(frame_pipeline));
	pass->wavefront = frames;
	bool failed = !frames || hipEventCreateWithFlags(&frames->inputs_ready, kSyncEventFlags) != hipSuccess
		|| hipEventCreateWithFlags(&frames->readers_done, kSyncEventFlags) != hipSuccess
		|| create_prepared_polygons(frames);
	for (int i = 0; i != VKR_MAX_FRAMES_IN_FLIGHT && !failed; ++i) failed = hipEventCreateWithFlags(&frames->contexts[i].done, kSyncEventFlags) != hipSuccess;
	if (failed) {
		printf("Failed to create the events of the frame pipeline.\n");
		destroy_wavefront(pass);
		return NULL;
	}
	frames->wide_stack_lds = environment_knob("VKR_WIDE_STACK_LDS", kWideStackLds, 4u, kWideStackLds);
	create_light_shafts(frames);
	// VKR_WIDE_REFILL: lanes of a tracing wave (four-wide tree) that have to be idle before they are handed the next rays,
	// once the wave has found its batches less than VKR_WIDE_REFILL_BELOW / 256 busy (wavefront_kernels.h; 256: from the
	// first batch on); 0: a batch of 64 rays is always walked to its end first (until round 4)
	frames->wide_refill = environment_knob("VKR_WIDE_REFILL", kWideRefillLanes, 0u, 64u);
	frames->wide_refill_below = environment_knob("VKR_WIDE_REFILL_BELOW", kWideRefillBelow, 0u, 256u);
	frames->wavefront_budget_mib = environment_knob("VKR_WAVEFRONT_BUDGET_MIB", 36864u, 64u, 262144u);
	frames->band_count = environment_knob("VKR_BAND_COUNT", 0u, 0u, 4096u);
	return frames;
}

// Slots a shading wave reserves per atomic (shade_params.ray_block): pays off when a lane
// queues many rays; with one or two per lane the unused slots would outnumber the rays.
// Unused slots of a wave's last block become null rays, a contiguous run that the tracing kernel
// skips a batch at a time.
static uint32_t ray_block_size(uint32_t max_terms) { return max_terms >= 8 ? 256u : 0u; }
// Arguments of the tracing kernels: lanes that must have a triangle waiting before a wave tests triangles
// (trace_shadow_rays_wide), and the refill threshold of the binary walk (trace_shadow_rays)
constexpr uint32_t kLeafBatch = 16;
constexpr uint32_t kRefillThreshold = 0;

static int ensure_spill(wavefront_buffers* w, uint32_t stack_need, uint32_t in_lds, uint32_t trace_threads) {
	size_t entries = stack_need > in_lds ? (size_t) (stack_need - in_lds) * trace_threads : 0;
	return grow_device_buffer(&w->spill, &w->spill_entries, entries, sizeof(uint32_t), "Failed to allocate %.1f MiB for the traversal stacks that do not fit into LDS.\n");
}

// Bytes per term slot of the streams every frame needs (visible value 12, code 1) and per ray slot (20)
static uint32_t queue_capacity_for(uint32_t thread_count, uint32_t max_terms) {
	// a queue sees every 512th wave (8 XCDs x 64 queues, waves dealt round-robin), every
	// lane of which may emit max_terms rays
	return ((thread_count / 64 + kRayQueueCount - 1) / kRayQueueCount + 1) * (64u * max_terms + ray_block_size(max_terms));
}

// bytes that ensure_wavefront() allocates for a launch of thread_count threads
// (with the light shafts' table: a verdict word per 8x8 patch and light and, with occluder lists, kShaftListMax entries each)
static double wavefront_bytes(uint32_t thread_count, uint32_t max_terms, uint32_t light_count, bool hidden_terms, bool base_color, uint32_t table_bytes_per_thread = 0) {
	double terms = (double) max_terms * thread_count;
	double shaft_pairs = (double) (thread_count / 64u) * light_count;
	return terms * (hidden_terms ? 24.0 : 12.0) + (double) ((max_terms + light_count + 2 + 3) & ~3u) * thread_count + (base_color ? 16.0 : 0.0) * thread_count
		+ 16.0 * thread_count + (double) queue_capacity_for(thread_count, max_terms) * kRayQueueCount * 20.0
		+ shaft_pairs * (4.0 + 4.0 * kShaftListMax * kShaftListEntry) + (double) table_bytes_per_thread * thread_count;
}

// `stream`: the stream the frame that uses these buffers is about to run on.  The counters are cleared
// THERE: the frame streams are non-blocking, i.e. not ordered behind a hipMemset on the null stream, and
// a frame that started before that memset landed had its queue sizes reset under its feet (found in
// round 3: the first frame of a fresh context lost a few rays).
static int ensure_wavefront(wavefront_buffers* w, uint32_t thread_count, uint32_t max_terms, uint32_t light_count, bool hidden_terms, bool base_color, hipStream_t stream) {
	uint32_t max_codes = max_terms + light_count + 2;
	size_t terms = (size_t) max_terms * thread_count;
	if (w->codes && w->thread_count == thread_count && w->max_terms == max_terms && w->max_codes == max_codes) {
		// (frames in flight may still use the other streams of this context: allocating does not disturb them)
		return (hidden_terms && grow_device_buffer(&w->terms_hidden, &w->hidden_term_count, terms, 12, "Failed to allocate %.1f MiB for the values of blocked terms.\n"))
			|| (base_color && grow_device_buffer(&w->base_color, &w->base_color_count, thread_count, sizeof(float4), "Failed to allocate the colours of the light display.\n"));
	}
	free_wavefront_buffers(w);
	w->thread_count = thread_count; w->max_terms = max_terms; w->max_codes = max_codes;
	// the record word of a ray: thread and code cursor (shade_params.h ray_record)
	uint32_t thread_bits = 1;
	while (thread_bits < 32 && (1ull << thread_bits) < thread_count) ++thread_bits;
	if (terms >= 0xFFFFFFFFull || (size_t) (max_codes + 3u) * thread_count >= 0xFFFFFFFFull || thread_bits >= 32 || ((uint64_t) max_codes << thread_bits) > 0xFFFFFFFFull) {
		printf("The wavefront ray queue would need more than 2^32 entries (%u threads x %u terms); render in more bands or use inline rays.\n", thread_count, max_terms);
		return 1;
	}
	w->thread_bits = thread_bits;
	w->queue_capacity = queue_capacity_for(thread_count, max_terms);
	size_t ray_slots = (size_t) w->queue_capacity * kRayQueueCount;
	// (codes are stored four to a word per thread: code_slot() in shade_params.h)
	if (hipMalloc(&w->codes, (size_t) ((max_codes + 3u) & ~3u) * thread_count) != hipSuccess
		|| hipMalloc(&w->terms_visible, terms * 12) != hipSuccess
		|| (hidden_terms && hipMalloc(&w->terms_hidden, terms * 12) != hipSuccess)
		|| (base_color && hipMalloc(&w->base_color, sizeof(float4) * (size_t) thread_count) != hipSuccess)
		|| hipMalloc(&w->ray_directions, ray_slots * 16) != hipSuccess
		|| hipMalloc(&w->ray_records, ray_slots * 4) != hipSuccess
		|| hipMalloc(&w->ray_origins, sizeof(float4) * (size_t) thread_count) != hipSuccess
		|| hipMalloc(&w->ray_queue_size, sizeof(uint32_t) * 2 * kRayCounterCount) != hipSuccess
		|| hipMemsetAsync(w->ray_queue_size, 0, sizeof(uint32_t) * 2 * kRayCounterCount, stream) != hipSuccess)
	{
		printf("Failed to allocate %.1f MiB for the wavefront ray queue and term streams.\n", wavefront_bytes(thread_count, max_terms, light_count, hidden_terms, base_color) / 1048576.0);
		free_wavefront_buffers(w);
		return 1;
	}
	w->hidden_term_count = hidden_terms ? terms : 0;
	w->base_color_count = base_color ? thread_count : 0;
	return 0;
}

extern "C" void mark_inputs_changed(application_t* app) {
	app->shading_pass.inputs_changed = 1;
	// (no pipeline yet: no verdict of an earlier arrangement exists either)
	if (app->shading_pass.wavefront) ++((frame_pipeline*) app->shading_pass.wavefront)->inputs_generation;
}

// The stream the next render_shading_pass() will run on if it is pipelined the way the last
// frame was (frame stream `next` of the pipeline), else device->stream
extern "C" void* get_next_frame_stream(const application_t* app) {
	const frame_pipeline* frames = (const frame_pipeline*) app->shading_pass.wavefront;
	if (!frames || !app->shading_pass.last_frame_in_flight || !frames->depth) return app->device.stream;
	return app->device.frame_streams[frames->next % frames->depth];
}

extern "C" int finish_frames(application_t* app) {
	frame_pipeline* frames = (frame_pipeline*) app->shading_pass.wavefront;
	if (!frames) return 0;
	int failed = 0;
	// (only device->stream's view changes: the order among the frames themselves is kept by
	// frame_context::recorded, which stays set)
	for (frame_context& c : frames->contexts)
		if (c.pending) {
			failed |= hip_failed(hipStreamWaitEvent((hipStream_t) app->device.stream, c.done, 0), "waiting for a frame in flight");
			c.pending = false;
		}
	return failed;
}

extern "C" void destroy_shading_pass(shading_pass_t* pass, const device_t* device) {
	// frames in flight still read the buffers that are freed below
	if (device && pass->wavefront) (void) wait_for_device(device);
	destroy_read_back(pass);
	destroy_constants_ring(pass, device);
	if (pass->ray_counter) (void) hipFree(pass->ray_counter);
	if (pass->pixel_materials) (void) hipFree(pass->pixel_materials);
	destroy_wavefront(pass);
	if (pass->timing_ring) {
		hipEvent_t* ring = (hipEvent_t*) pass->timing_ring;
		for (uint32_t i = 0; i != kTimingEvents * pass->timing_ring_size; ++i) if (ring[i]) (void) hipEventDestroy(ring[i]);
		free(ring);
	}
	memset(pass, 0, sizeof(*pass));
}

// The same legality rules the reference enforces in its GUI
// (src/user_interface.cpp:90-180), as hard errors.
static int validate_settings(const application_t* app) {
	const render_settings_t* s = &app->render_settings;
	const scene_specification_t* spec = &app->scene_specification;
	int technique = technique_index(s);
	if (technique < 0) {
		printf("Invalid polygon sampling technique %d.\n", (int) s->polygon_sampling_technique);
		return 1;
	}
	bool is_psa = is_projected_solid_angle(technique);
	// An out-of-range strategy selects none of the strategy defines of the reference, i.e.
	// the combined diffuse + specular preparation with no estimator behind it.  That is
	// only meaningful with an error display (the reference's own experiment table does it,
	// experiment_list.c:107); everything else is refused.
	bool strategy_in_range = s->sampling_strategies < sampling_strategies_count;
	if ((!strategy_in_range && !(s->error_display != error_display_none && is_psa)) || s->mis_heuristic >= mis_heuristic_count) {
		printf("Invalid sampling strategy or MIS heuristic.\n");
		return 1;
	}
	bool needs_specular = strategy_in_range && has_specular_technique(s);
	if ((technique == kTechniqueBaseline || technique == kTechniqueAreaTurk || technique == kTechniqueHartBilinear || technique == kTechniqueHartBilinearClipping
			|| technique == kTechniqueHartBiquadratic || technique == kTechniqueHartBiquadraticClipping)
		&& s->sampling_strategies != sampling_strategies_diffuse_only)
	{
		printf("The baseline, area sampling and cosine warp techniques only exist for the diffuse-only sampling strategy (as in the reference shader).\n");
		return 1;
	}
	if (needs_specular && !is_psa) {
		printf("Sampling strategies with LTC importance sampling require projected solid angle sampling.\n");
		return 1;
	}
	if ((s->mis_heuristic == mis_heuristic_weighted || s->mis_heuristic == mis_heuristic_optimal_clamped || s->mis_heuristic == mis_heuristic_optimal)
		&& s->sampling_strategies == sampling_strategies_diffuse_ggx_mis)
	{
		printf("The weighted and optimal MIS heuristics are only defined for the diffuse+specular MIS strategy.\n");
		return 1;
	}
	if (s->error_display >= error_display_count) {
		printf("Invalid error display mode.\n");
		return 1;
	}
	if (technique == kTechniquePsaArvo && s->error_display == error_display_diffuse_forward) {
		printf("Arvo's sampler only defines the backward errors (the reference shader does not compile with the forward error either).\n");
		return 1;
	}
	if (s->sample_count == 0) {
		printf("The sample count must be positive.\n");
		return 1;
	}
	for (uint32_t i = 0; i != spec->polygonal_light_count; ++i) {
		const polygonal_light_t* light = &spec->polygonal_lights[i];
		if (light->vertex_count < 3 || light->vertex_count > 7) {
			printf("Polygonal light %u has %u vertices; the clipping and sorting code covers 3 to 7.\n", i, light->vertex_count);
			return 1;
		}
		if (light->texturing_technique < 0 || light->texturing_technique >= polygon_texturing_count) {
			printf("Polygonal light %u has the invalid texturing technique %d.\n", i, (int) light->texturing_technique);
			return 1;
		}
	}
	return 0;
}

static int create_timing_ring(shading_pass_t* pass) {
	pass->timing_ring_size = 256;
	// per timed frame: start, end of the shading kernel, end of the frame
	hipEvent_t* ring = (hipEvent_t*) calloc(kTimingEvents * pass->timing_ring_size, sizeof(hipEvent_t));
	pass->timing_ring = ring;
	for (uint32_t i = 0; i != kTimingEvents * pass->timing_ring_size; ++i)
		if (hip_failed(hipEventCreateWithFlags(&ring[i], hipEventReleaseToDevice), "creating timing events")) return 1;
	return 0;
}

extern "C" int create_shading_pass(shading_pass_t* pass, application_t* app) {
	int32_t arithmetic_mode = pass->arithmetic_mode, inline_rays = pass->inline_rays, binary_traversal = pass->binary_traversal;
	uint32_t band_count = pass->band_count;
	void* wait_before_next_frame = pass->wait_before_next_frame;
	uint32_t timing_stride = pass->timing_stride, frames_in_flight = pass->frames_in_flight;
	memset(pass, 0, sizeof(*pass));
	pass->timing_stride = timing_stride;
	pass->frames_in_flight = frames_in_flight;
	pass->inputs_changed = 1;
	if (arithmetic_mode < 0 || arithmetic_mode >= arithmetic_mode_count) {
		printf("Invalid arithmetic mode %d (0: libm, 1: fast, 2: polynomial).\n", arithmetic_mode);
		return 1;
	}
	pass->arithmetic_mode = arithmetic_mode;
	pass->wait_before_next_frame = wait_before_next_frame;
	pass->band_count = band_count;
	pass->inline_rays = inline_rays ? 1 : 0;
	pass->binary_traversal = binary_traversal ? 1 : 0;
	pass->variant = -1;
	const device_t* device = &app->device;
	if (validate_settings(app)) return 1;
	pass->use_ray_tracing = app->render_settings.trace_shadow_rays && app->scene.acceleration_structure.triangle_vertices != NULL;
	if (app->render_settings.trace_shadow_rays && !pass->use_ray_tracing)
		printf("Shadow rays were requested but the scene has no acceleration structure; rendering without shadows.\n");
	pass->max_polygon_vertex_count = get_max_polygon_vertex_count(&app->scene_specification, &app->render_settings);
	pass->variant = (int32_t) app->render_settings.sampling_strategies * kTechniqueCount + technique_index(&app->render_settings);
	pass->constants_size = get_constant_buffer_size(app);
	if (create_constants_ring(pass, device) || create_timing_ring(pass))
	{
		printf("Failed to create the shading pass.\n");
		destroy_shading_pass(pass, device);
		return 1;
	}
	return 0;
}

// (schedule: the caller's copy of the application's)
static void fill_tile_schedule(shade_params& p, tile_schedule_t schedule, uint32_t& grid_blocks) {
	if (schedule.rank_count <= 1) { schedule.rank = 0; schedule.rank_count = 1; }
	// tile_size 0: automatic.  The blocks of a tile are consecutive in the launch, so the tile size decides which 16x16 blocks
	// are in flight together: raster order of blocks (tile 16) spreads the resident waves over a band of the whole frame width,
	// tiles of 64 keep them in compact squares.  Measured on one GPU, frames bit-identical (profiles/r10r/tile_order.jsonl,
	// tile 16 / 32 / 64 / 128): config 3 1.157 / 1.136 / 1.129 / 1.152 ms, large scene 3.96 / 3.90 / 3.90 / 3.95, target shape
	// 0.432 / 0.425 / 0.428 / 0.429, config 2 0.140 / 0.139 / 0.138 / 0.139; the 3840x2160 frame of config 4 16.33 / 16.59 /
	// 16.56 / 16.20: 64 up to three megapixels, 128 above.
	// (only where the tile size does not shape the output: one rank that renders in place)
	if (schedule.tile_size == 0 && schedule.rank_count == 1 && !schedule.slab_layout) schedule.tile_size = ((uint64_t) p.width * p.height <= 3145728ull) ? 64u : 128u;
	if (schedule.tile_size < 16) schedule.tile_size = 16;
	schedule.tile_size = (schedule.tile_size + 15) & ~15u;
	p.tile_size = schedule.tile_size;
	p.rank = schedule.rank;
	p.rank_count = schedule.rank_count;
	p.slab_layout = (schedule.rank_count > 1 || schedule.slab_layout) ? 1u : 0u;
	p.tiles_x = (p.width + p.tile_size - 1) / p.tile_size;
	uint32_t tiles_y = (p.height + p.tile_size - 1) / p.tile_size;
	p.tile_count = p.tiles_x * tiles_y;
	uint32_t own_tiles = (p.tile_count + p.rank_count - 1 - p.rank) / p.rank_count;
	uint32_t blocks_per_tile = (p.tile_size / 16) * (p.tile_size / 16);
	grid_blocks = own_tiles * blocks_per_tile;
}

uint64_t slab_tiling(const application_t* app, uint32_t rank, shade_params& p) {
	memset(&p, 0, sizeof(p));
	p.width = app->swapchain.extent.width;
	p.height = app->swapchain.extent.height;
	tile_schedule_t schedule = app->tile_schedule;
	schedule.rank = rank;
	uint32_t grid_blocks = 0;
	fill_tile_schedule(p, schedule, grid_blocks);
	return (uint64_t) grid_blocks * 256;
}

// the parameters of a frame that come straight from the application
static void fill_frame_inputs(const application_t* app, void* out_radiance, shade_params& p) {
	memset(&p, 0, sizeof(p));
	p.light_count = app->scene_specification.polygonal_light_count;
	p.max_light_vertex_count = get_max_polygonal_light_vertex_count(&app->scene_specification);
	p.sample_count = app->render_settings.sample_count;
	p.mis_heuristic = (int32_t) app->render_settings.mis_heuristic;
	p.show_polygonal_lights = app->render_settings.show_polygonal_lights ? 1 : 0;
	p.positions = (const uint2*) app->scene.mesh.positions;
	p.normals_and_tex_coords = (const uint2*) app->scene.mesh.normals_and_tex_coords;
	p.material_indices = (const uint8_t*) app->scene.mesh.material_indices;
	p.material_constants = (const float*) app->scene.materials.constants;
	p.visibility = (const uint32_t*) app->render_targets.visibility_buffer;
	p.out_radiance = (float4*) (out_radiance ? out_radiance : app->render_targets.radiance);
	p.width = app->swapchain.extent.width;
	p.height = app->swapchain.extent.height;
	p.ltc_rgba = (const uint2*) app->ltc_table.device_rgba;
	p.ltc_rg = (const uint32_t*) app->ltc_table.device_rg;
	p.ltc_resolution = app->ltc_table.roughness_count;
	p.ltc_layer_count = app->ltc_table.fresnel_count;
	p.noise = (const uint2*) app->noise_table.device_data;
	p.noise_width = app->noise_table.resolution.width;
	p.noise_height = app->noise_table.resolution.height;
	p.bvh = make_bvh_view(&app->scene.acceleration_structure);
}

// Error display (ERROR_DISPLAY_DIFFUSE / _SPECULAR / ERROR_INDEX, main.c:728-750): only
// the projected solid angle paths look at these flags, and the specular display
// exists only where the specular technique is prepared.  The program returns
// before it samples, so no ray is ever traced.
static void plan_error_display(const application_t* app, frame_plan* f) {
	int display = (int) app->render_settings.error_display;
	f->error_mode = kErrorNone;
	if (display != error_display_none && is_projected_solid_angle(f->technique)) {
		bool specular = display == error_display_specular_backward || display == error_display_specular_backward_scaled || display == error_display_specular_forward;
		f->error_mode = specular ? (has_specular_technique(&app->render_settings) ? kErrorSpecular : kErrorNone) : kErrorDiffuse;
	}
	if (f->error_mode == kErrorNone) return;
	f->ray_mode = kRaysNone;
	f->p.error_index = (display == error_display_diffuse_backward || display == error_display_specular_backward) ? 0u
		: ((display == error_display_diffuse_backward_scaled || display == error_display_specular_backward_scaled) ? 1u : 2u);
	// the constants that the GLSL compiler folds in error_to_color (shading_pass.frag.glsl:81-89)
	f->p.error_max = powf(10.0f, 5.0f - 0.01f);
	f->p.error_scale = 20.0f / ((5.0f - 0.0f) * log2f(10.0f));
}

// The checks of a frame and the decisions that need no HIP call: one launch of the whole schedule until plan_bands()
static int plan_frame(application_t* app, void* out_radiance, frame_plan* f) {
	const shading_pass_t* pass = &app->shading_pass;
	if (pass->variant < 0 || !pass->constants_device) {
		printf("render_shading_pass() needs a shading pass created by create_shading_pass().\n");
		return 1;
	}
	// settings may have been edited since create_shading_pass(): the same legality rules apply, and the
	// launcher tables below are indexed with them
	if (validate_settings(app)) return 1;
	memset(f, 0, sizeof(*f));
	f->strategy = (int) app->render_settings.sampling_strategies;
	f->technique = technique_index(&app->render_settings);
	if (get_constant_buffer_size(app) != pass->constants_size
		|| get_max_polygon_vertex_count(&app->scene_specification, &app->render_settings) != pass->max_polygon_vertex_count
		|| (int32_t) app->render_settings.sampling_strategies * kTechniqueCount + f->technique != pass->variant)
	{
		printf("Lights or render settings changed in a way that needs a different kernel variant. Recreate the shading pass (the reference recompiles its shader in this situation, main.c:1833-1881).\n");
		return 1;
	}
	shade_params& p = f->p;
	fill_frame_inputs(app, out_radiance, p);
	if (!p.positions || !p.visibility || !p.out_radiance || !p.ltc_rgba || !p.noise || !p.material_constants) {
		printf("render_shading_pass() needs a loaded scene, LTC table, noise table and render targets on the device.\n");
		return 1;
	}
	if (p.width != app->render_targets.extent.width || p.height != app->render_targets.extent.height) {
		printf("The render targets do not match the swapchain extent.\n");
		return 1;
	}
	fill_tile_schedule(p, app->tile_schedule, f->grid_blocks);
	f->ray_mode = !pass->use_ray_tracing ? kRaysNone : (pass->inline_rays ? kRaysInline : kRaysDeferred);
	plan_error_display(app, f);
	if (f->error_mode == kErrorNone && f->strategy >= (int) sampling_strategies_count) {
		// (an out-of-range strategy is only legal together with an error display that is really shown:
		// a specular display without the combined path shows nothing and would index past the launcher table)
		printf("No kernel variant exists for sampling strategy %d without an error display.\n", f->strategy);
		return 1;
	}
	// (the same as the light vertex count plus one for the techniques that clip, host/constants.c, checked above)
	f->capacity = (int) pass->max_polygon_vertex_count;
	const bool specular = has_specular_technique(&app->render_settings);
	f->table_in_memory = specular && (f->technique == kTechniquePsa || f->technique == kTechniquePsaBiased) && f->error_mode == kErrorNone && psa_table_in_memory(f->capacity);
	f->table_bytes_per_workgroup = f->table_in_memory ? psa_table_memory_bytes_per_workgroup(f->capacity) : 0u;
	f->use_wide_tree = app->scene.acceleration_structure.wide_nodes && !pass->binary_traversal;
	f->max_terms = 2u * p.light_count * p.sample_count;
	if (f->ray_mode == kRaysDeferred && specular && ray_block_size(f->max_terms)) f->ray_mode = kRaysDeferredBlocks;
	// values of blocked terms exist for the plain optimal heuristic only (its estimate is not proportional
	// to the integrand); a colour before the sampled terms only with the light display
	f->hidden_terms = app->render_settings.mis_heuristic == mis_heuristic_optimal && f->strategy == (int) sampling_strategies_diffuse_specular_mis;
	f->base_color = p.show_polygonal_lights != 0;
	f->depth = f->band_count = 1;
	f->blocks_per_band = f->grid_blocks;
	// textured scene: sample the material textures of every pixel first (same stream)
	f->textured = app->scene.materials.textured && app->scene.materials.texture_descriptors;
	if (f->textured) {
		p.texture_descriptors = (const uint32_t*) app->scene.materials.texture_descriptors;
		p.texels = (const uint32_t*) app->scene.materials.texels;
		p.srgb_table = (const float*) app->scene.materials.srgb_table;
	}
	// slab layout: every thread of the grid owns a slot; full-frame layout: the pixels
	f->frame_output_bytes = sizeof(float4) * (p.slab_layout ? (size_t) f->grid_blocks * 256u : (size_t) p.width * p.height);
	return 0;
}

// Launches with wavefront rays may run n at a time: launch k on frame stream k mod n with
// its own buffers, so that the (latency-bound) tracing of one launch overlaps the
// (VALU-bound) shading of the next ones.  Everything else runs on device->stream, behind
// any launch that is still in flight.
// A frame is one launch - or several, "bands" of consecutive 16x16 blocks of the rank's schedule,
// when the wavefront buffers of the whole frame (sized for the worst case: every sample of every
// light on every pixel queues a ray) would be larger than the budget: a band is shaded, traced and
// resolved like a small frame, with buffers sized for the band, and the bands of one frame - and of
// the next frames - overlap on the frame streams exactly like whole frames do.
static int plan_bands(application_t* app, frame_plan* f) {
	const device_t* device = &app->device;
	frame_pipeline* frames = f->frames = ensure_frames(&app->shading_pass);
	if (!frames) return 1;
	// (a textured scene has one per-pixel material buffer: one frame at a time)
	uint32_t depth = app->shading_pass.frames_in_flight < VKR_MAX_FRAMES_IN_FLIGHT ? app->shading_pass.frames_in_flight : VKR_MAX_FRAMES_IN_FLIGHT;
	// (the device creates four frame streams; a deeper pipeline gets the others now)
	if (depth >= 2 && !device->frame_streams[depth - 1] && vkr_ensure_frame_streams(&app->device, depth)) return 1;
	while (depth >= 2 && !device->frame_streams[depth - 1]) --depth;
	if (depth < 1) depth = 1;
	f->pipelined = depth >= 2 && !app->scene.materials.textured;
	f->depth = f->pipelined ? depth : 1u;
	// Bands: as few as keep all sets of buffers in flight within the budget, each at least
	// kMinBandBlocks blocks (a launch has to fill the GPU several times over), whole groups of 8 blocks
	// (shade_grid_size).  pass->band_count / VKR_BAND_COUNT force a number.
	const double budget = (double) frames->wavefront_budget_mib * 1048576.0;
	const uint32_t kMinBandBlocks = 4096, grid_blocks = f->grid_blocks;
	uint32_t wanted = app->shading_pass.band_count ? app->shading_pass.band_count : frames->band_count;
	if (!wanted) {
		wanted = 1;
		while (f->depth * wavefront_bytes(((grid_blocks + wanted - 1) / wanted) * 256u, f->max_terms, f->p.light_count, f->hidden_terms, f->base_color, f->table_bytes_per_workgroup / 64u) > budget
			&& (grid_blocks + wanted) / (wanted + 1) >= kMinBandBlocks)
			++wanted;
	}
	f->blocks_per_band = (((grid_blocks + wanted - 1) / wanted) + 7u) & ~7u;
	if (f->blocks_per_band == 0) f->blocks_per_band = 8;
	f->band_count = (grid_blocks + f->blocks_per_band - 1) / f->blocks_per_band;
	if (f->band_count == 0) f->band_count = 1;
	// The tracing kernels are persistent: a number of waves per SIMD on every CU, each lane strides over the queues.
	// Small launches (round 5, profiles/r07f): a rank's slab at N = 8 is 4 080 shading waves on 3 072 wave slots.  Its
	// kernels then last about as long as their slowest wave, and what is launched for a whole frame - 8 192 tracing
	// waves for 230 k rays, shaft walks of up to 72 steps - is mostly waiting: with 2 tracing waves per SIMD and walks
	// that give up after 12 steps (more rays traced, a shorter chain of kernels) the slab of config 3 takes 0.177
	// instead of 0.199 ms, the target shape's 0.070 instead of 0.084; a quarter of the frame (8 160 waves) 0.316
	// instead of 0.333.  The whole frame (32 640 waves) loses with either: 1.150 -> 1.176 ms with 12 steps.
	// Otherwise eight waves per SIMD where a lane queues eight rays or more, four where it queues fewer (measured at config 2,
	// whose 0.9 M rays are a batch or two per wave: 0.129 -> 0.121 ms per frame).
	const uint32_t compute_units = (uint32_t) (device->compute_unit_count > 0 ? device->compute_unit_count : 256);
	const uint32_t launch_waves = shade_grid_size(f->blocks_per_band);
	const uint32_t small_launch_waves = launch_waves < 6144u ? 2u : (launch_waves < 12288u ? 4u : 0u);
	f->trace_blocks = compute_units * (small_launch_waves ? small_launch_waves : (f->max_terms >= 8u ? 8u : 4u));
	// (queues of XCD x are only served by workgroups b with b % 8 == x)
	f->trace_blocks = (f->trace_blocks + 7u) & ~7u;
	f->p.ray_block = f->ray_mode == kRaysDeferredBlocks ? ray_block_size(f->max_terms) : 0u;
	f->p.refill_threshold = kRefillThreshold;
	// (the kept prepared polygons count against the budget beside the wavefront buffers of the frame's one launch)
	plan_prepared_polygons(app, f, f->depth * wavefront_bytes(f->blocks_per_band * 256u, f->max_terms, f->p.light_count, f->hidden_terms, f->base_color, 0u), budget);
	return 0;
}

// Orders the frame among the frames in flight: a frame outside the pipeline runs behind all of them (on device->stream); a
// pipelined one starts afresh at another depth, and its frame streams wait for inputs that changed on device->stream
static int join_frame_pipeline(application_t* app, frame_plan* f) {
	shading_pass_t* pass = &app->shading_pass;
	if (!f->pipelined) {
		if (finish_frames(app)) return 1;
		// (no wavefront buffers, but the table in device memory lives with them: context 0)
		if (!is_deferred(f->ray_mode) && f->table_in_memory && !(f->frames = ensure_frames(pass))) return 1;
		return 0;
	}
	frame_pipeline* frames = f->frames;
	if (frames->depth != f->depth) {
		// another pipeline depth: contexts and streams pair up differently, start afresh
		if (frames->depth && wait_for_device(&app->device)) return 1;
		for (frame_context& c : frames->contexts) c.recorded = c.pending = false;
		frames->depth = f->depth;
		frames->next = 0;
	}
	if (pass->inputs_changed) {
		// Inputs that were produced on device->stream (visibility pass, uploads): all frame
		// streams wait for them once.  Frames do not wait for anything else on
		// device->stream - if they did, a consumer of frame k there would hold back frame k + 1.
		if (hip_failed(hipEventRecord(frames->inputs_ready, (hipStream_t) app->device.stream), "marking the inputs")) return 1;
		for (uint32_t i = 0; i != f->depth; ++i)
			if (hip_failed(hipStreamWaitEvent((hipStream_t) app->device.frame_streams[i], frames->inputs_ready, 0), "waiting for the inputs")) return 1;
		pass->inputs_changed = 0;
	}
	return 0;
}

// The per-pixel materials of a textured scene, which resolve_materials() writes, and the light textures
static int bind_textures(application_t* app, frame_plan* f) {
	shading_pass_t* pass = &app->shading_pass;
	shade_params& p = f->p;
	size_t needed = sizeof(float) * 8 * (size_t) p.width * p.height;
	if (f->textured && pass->pixel_materials_size != needed) {
		if (wait_for_device(&app->device)) return 1;
		(void) hipFree(pass->pixel_materials);
		pass->pixel_materials = NULL;
		pass->pixel_materials_size = 0;
		if (hip_failed(hipMalloc(&pass->pixel_materials, needed), "allocating the per-pixel materials")) return 1;
		pass->pixel_materials_size = needed;
	}
	// light textures: bound whenever a light asks for one (the technique lives in the constants)
	for (uint32_t i = 0; i != app->scene_specification.polygonal_light_count; ++i) {
		const polygonal_light_t* light = &app->scene_specification.polygonal_lights[i];
		if (light->texturing_technique == polygon_texturing_none) continue;
		if (!app->light_textures.descriptors || light->texture_index >= app->light_textures.texture_count) {
			printf("Polygonal light %u uses a texture but the light textures have not been created for the current lights. Call create_and_assign_light_textures() first.\n", i);
			return 1;
		}
		p.light_texture_descriptors = (const uint4*) app->light_textures.descriptors;
		p.light_texels = (const float4*) app->light_textures.texels;
	}
	return 0;
}

// Band step 1: a band with wavefront rays takes a frame context - the next one in turn, on its frame stream, when the frame
// is pipelined - and its buffers; the polygon tables in device memory belong to that context or to device->stream
static int take_frame_context(application_t* app, frame_plan* f, frame_context** out_frame, hipStream_t* stream) {
	frame_pipeline* frames = f->frames;
	shade_params& p = f->p;
	frame_context* frame = NULL;
	if (is_deferred(f->ray_mode)) {
		uint32_t index = 0;
		if (f->pipelined) {
			index = frames->next;
			frames->next = (index + 1) % f->depth;
			*stream = (hipStream_t) app->device.frame_streams[index];
		}
		frame = &frames->contexts[index];
		frames->last = index;
		if (ensure_wavefront(&frame->buffers, f->blocks_per_band * 256u, f->max_terms, p.light_count, f->hidden_terms, f->base_color, *stream)) return 1;
		if (f->use_wide_tree && ensure_spill(&frame->buffers, app->scene.acceleration_structure.wide_stack_need, frames->wide_stack_lds, f->trace_blocks * 256u)) return 1;
		const wavefront_buffers* w = &frame->buffers;
		p.codes = w->codes; p.terms_visible = w->terms_visible; p.terms_hidden = w->terms_hidden; p.base_color = w->base_color;
		p.ray_directions = w->ray_directions; p.ray_records = w->ray_records; p.ray_origins = w->ray_origins; p.ray_queue_size = w->ray_queue_size;
		p.thread_count = w->thread_count; p.max_terms = w->max_terms; p.max_codes = w->max_codes;
		p.ray_queue_capacity = w->queue_capacity; p.ray_thread_bits = w->thread_bits;
	}
	*out_frame = frame;
	if (f->table_in_memory) {
		// a region per workgroup of the launch, in the launch's own buffers (shade_params.h psa_table_in_memory)
		wavefront_buffers* owner = frame ? &frame->buffers : &frames->device_stream_buffers;
		const size_t bytes = (size_t) shade_grid_size(f->blocks_per_band) * f->table_bytes_per_workgroup;
		if (grow_device_buffer(&owner->psa_table_memory, &owner->psa_table_bytes, bytes, 1, "Failed to allocate %.1f MiB for the polygon tables that do not fit into LDS.\n")) return 1;
		p.psa_table_memory = owner->psa_table_memory;
	}
	app->shading_pass.last_frame_stream = *stream;
	return 0;
}

// Band step 2: the band's stream waits for the caller's event, and for the constants, which are uploaded if they changed
static int upload_band_constants(application_t* app, frame_plan* f, uint32_t band, hipEvent_t caller_event, hipStream_t stream) {
	// (a target that earlier work of the caller still reads: every stream that writes it waits)
	if (caller_event && hip_failed(hipStreamWaitEvent(stream, caller_event, 0), "waiting for the caller's event")) return 1;
	// (wavefront rays: the resolve kernel of the frame's first launch stores the count instead)
	f->p.first_launch_of_frame = band == 0 ? 1u : 0u;
	if (band == 0 && f->p.ray_counter && !is_deferred(f->ray_mode) && hip_failed(hipMemsetAsync(f->p.ray_counter, 0, sizeof(unsigned long long), stream), "clearing the ray counter")) return 1;
	if (upload_constants(app, stream)) return 1;
	f->p.constants = (const uint8_t*) app->shading_pass.constants_device;
	return 0;
}

// Band step 3 (the first band of a textured frame): the materials of every pixel, from the material textures
static int resolve_materials(application_t* app, shade_params& p, hipStream_t stream) {
	shading_pass_t* pass = &app->shading_pass;
	if (g_resolve_launchers[pass->arithmetic_mode](&p, (float*) pass->pixel_materials, stream)) {
		printf("Launching the material resolve kernel failed.\n");
		return 1;
	}
	p.pixel_materials = (const float*) pass->pixel_materials;
	return 0;
}

// Band step 5: the shading kernel, or the error display's; < 0: no such kernel variant was built
static int launch_shading(const application_t* app, const frame_plan* f, hipStream_t stream) {
	const int mode = app->shading_pass.arithmetic_mode;
	const shade_params* p = &f->p;
	if (f->error_mode != kErrorNone)
		return g_error_launchers[mode](has_specular_technique(&app->render_settings), f->technique, f->capacity, f->error_mode, p, p->block_count, stream);
	if (f->prepared_mode != kPreparedPlain) return launch_prepared_shading(app, f, stream);
	return g_launchers[mode + (p->light_texture_descriptors ? 3 : 0)][f->strategy](f->technique, f->capacity, f->ray_mode, p, p->block_count, stream);
}

// Band step 6: the tracing kernel of the band's queued rays
static void launch_tracing(const application_t* app, const frame_plan* f, const frame_context* frame, hipStream_t stream) {
	const frame_pipeline* frames = f->frames;
	const shade_params& p = f->p;
	ray_stream rays = {p.ray_directions, p.ray_records, p.ray_origins, p.ray_queue_size, p.ray_queue_capacity, p.ray_thread_bits, p.thread_count};
	if (f->use_wide_tree) {
		const uint4* wide_nodes = (const uint4*) app->scene.acceleration_structure.wide_nodes;
		// single-wave workgroups where a lane queues many rays and the shading kernel runs three waves
		// per SIMD (wavefront_kernels.h has the measurements)
		if (f->ray_mode == kRaysDeferredBlocks && f->capacity <= 7) {
			trace_shadow_rays_wide<64><<<f->trace_blocks * 4u, 64, 0, stream>>>(p.bvh, wide_nodes, rays, p.ray_queue_size + kRayQueueCount, p.codes, frame->buffers.spill, kLeafBatch, frames->wide_stack_lds, frames->wide_refill, frames->wide_refill_below);
		}
		else {
			trace_shadow_rays_wide<256><<<f->trace_blocks, 256, 0, stream>>>(p.bvh, wide_nodes, rays, p.ray_queue_size + kRayQueueCount, p.codes, frame->buffers.spill, kLeafBatch, frames->wide_stack_lds, frames->wide_refill, frames->wide_refill_below);
		}
	}
	else
		trace_shadow_rays<<<f->trace_blocks, 256, 0, stream>>>(p.bvh, rays, p.ray_queue_size + kRayQueueCount, p.codes, p.refill_threshold);
}

// Orders a write of the frame's output on `stream`, in front of the resolve kernel with wavefront rays and in front of the
// shading kernel otherwise (such a frame is never pipelined)
static void order_output_write(shading_pass_t* pass, const frame_plan* f, frame_context* frame, uint32_t band, hipStream_t stream) {
	const void* target = f->p.out_radiance;
	if (f->pipelined) {
		frame_pipeline* frames = f->frames;
		// launches in flight may write the same target: keep their order there
		// (the launch before this one ran in the context before this one)
		// (whether device->stream has already been made to wait for that launch - finish_frames() -
		// says nothing about this stream)
		frame_context* previous = &frames->contexts[(frames->last + frames->depth - 1u) % frames->depth];
		// (bands of one frame, and frames that share a target)
		// (a caller's ring of targets need not have the length of the pipeline: every other context one of whose recent
		// launches wrote this target comes first)
		for (uint32_t c = 0; c != frames->depth; ++c) {
			frame_context* other = &frames->contexts[c];
			if (other == frame || !other->recorded) continue;
			bool same = other == previous && band != 0;
			for (const void* written : other->targets) same = same || written == target;
			if (same) (void) hipStreamWaitEvent(stream, other->done, 0);
		}
		frame->targets[frame->target_cursor++ % 8u] = target;
		// ... and behind whatever still reads the target on device->stream (output encoding)
		if (frame->readers_seen != frames->readers_generation) {
			(void) hipStreamWaitEvent(stream, frames->readers_done, 0);
			frame->readers_seen = frames->readers_generation;
		}
	}
	wait_for_read_backs_of(pass, target, f->frame_output_bytes, stream);
}

// Band step 8 (the last band, render_shading_pass_encoded()): the frame or slab as packed RGB8, on the band's stream
static int encode_frame_rgb8(application_t* app, const frame_plan* f, void* out_rgb8, hipStream_t stream) {
	// (the resolves of the bands are chained, so the last band's stream has seen them all)
	uint64_t pixels = f->frame_output_bytes / sizeof(float4);
	if (pixels % 4 != 0) {
		printf("The frame cannot be encoded as packed RGB8 (its pixel count has to be a multiple of four).\n");
		return 1;
	}
	wait_for_read_backs_of(&app->shading_pass, out_rgb8, (size_t) pixels * 3u, stream);
	launch_encode_rgb8(f->p.out_radiance, out_rgb8, pixels, app->screenshot.frame_bits, 0, stream);
	return hipGetLastError() != hipSuccess;
}

// out_rgb8: the frame (or slab) is also encoded as packed RGB8 on the stream it was rendered on
static int render_pass(application_t* app, void* out_radiance, void* out_rgb8) {
	shading_pass_t* pass = &app->shading_pass;
	frame_plan f;
	if (plan_frame(app, out_radiance, &f)) return 1;
	shade_params& p = f.p;
	if (pass->use_ray_tracing) {
		// (sixteen counters, one per frame in turn: see below)
		if (!pass->ray_counter && hip_failed(hipMalloc(&pass->ray_counter, 16 * sizeof(unsigned long long)), "allocating the ray counters")) return 1;
		p.ray_counter = (unsigned long long*) pass->ray_counter;
	}
	if ((is_deferred(f.ray_mode) && plan_bands(app, &f)) || join_frame_pipeline(app, &f)) return 1;
	pass->last_frame_traced_rays = f.ray_mode != kRaysNone;
	pass->last_frame_in_flight = f.pipelined ? f.depth : 0u;
	pass->last_band_count = f.band_count;
	if (bind_textures(app, &f)) return 1;
	// every timing_stride-th frame is bracketed by events: start, end of the (last band's) shading
	// kernel, end of the frame (an event record costs about 5 us of idle time on the stream, a tenth
	// of a config-2 frame for the pair)
	const uint32_t slot = pass->timing_cursor % pass->timing_ring_size;
	const bool timed = pass->timing_stride <= 1 || pass->frame_counter % pass->timing_stride == 0;
	// rays of this frame: one of sixteen counters, taken in turn, so that the bands of this frame never
	// meet those of a frame that is still in flight (at most eight launches are)
	if (p.ray_counter) p.ray_counter += pass->frame_counter % 16u;
	++pass->frame_counter;
	hipEvent_t caller_event = (hipEvent_t) pass->wait_before_next_frame;
	pass->wait_before_next_frame = NULL;
	hipStream_t stream = (hipStream_t) app->device.stream;
	frame_context* frame = NULL;
	int status = 0;
	for (uint32_t band = 0; band != f.band_count && status == 0; ++band) {
		p.first_block = band * f.blocks_per_band;
		p.block_count = f.grid_blocks - p.first_block < f.blocks_per_band ? f.grid_blocks - p.first_block : f.blocks_per_band;
		if (take_frame_context(app, &f, &frame, &stream) || upload_band_constants(app, &f, band, caller_event, stream)) return 1;
		// (the first event of a timed frame: everything the frame launches lies behind it)
		if (timed && band == 0) (void) hipEventRecord(timing_event(pass, slot, kTimingFrameStart), stream);
		if ((f.textured && band == 0 && resolve_materials(app, p, stream)) || run_light_shafts(app, &f, frame, stream)) return 1;
		// (a frame without wavefront rays writes its output from the shading kernel)
		if (!is_deferred(f.ray_mode)) order_output_write(pass, &f, frame, band, stream);
		// (the second event of a timed frame: the shading kernel itself begins here, behind the shaft kernel)
		if (timed && band == 0) (void) hipEventRecord(timing_event(pass, slot, kTimingShadingStart), stream);
		if (choose_prepared_mode(app, &f, frame, stream)) return 1;
		status = launch_shading(app, &f, stream);
		note_prepared_launch(app, &f, status, stream);
		if (timed && band + 1 == f.band_count) (void) hipEventRecord(timing_event(pass, slot, kTimingShadingEnd), stream);
		if (status == 0 && is_deferred(f.ray_mode)) {
			launch_tracing(app, &f, frame, stream);
			order_output_write(pass, &f, frame, band, stream);
			resolve_shadow_terms_and_reset<<<p.block_count, 256, 0, stream>>>(p);
			status = hipGetLastError() != hipSuccess;
		}
		if (status == 0 && out_rgb8 && band + 1 == f.band_count) status = encode_frame_rgb8(app, &f, out_rgb8, stream);
		// band step 9: later frames that write the same target are ordered behind this event
		if (status == 0 && f.pipelined) {
			(void) hipEventRecord(frame->done, stream);
			frame->pending = frame->recorded = true;
		}
	}
	if (timed) {
		(void) hipEventRecord(timing_event(pass, slot, kTimingFrameEnd), stream);
		++pass->timing_cursor;
	}
	if (status < 0) {
		printf("No kernel variant was built for strategy %d, technique %d, vertex capacity %d.\n", f.strategy, f.technique, f.capacity);
		return 1;
	}
	if (status > 0) {
		// the resolve kernel did not run, so the ray queues may not be empty
		if (frame && frame->buffers.ray_queue_size) (void) hipMemsetAsync(frame->buffers.ray_queue_size, 0, sizeof(uint32_t) * kRayCounterCount, stream);
		printf("Launching the shading kernel failed: %s\n", hipGetErrorString(hipGetLastError()));
		return 1;
	}
	return 0;
}

extern "C" int render_shading_pass(application_t* app, void* out_radiance) {
	return render_pass(app, out_radiance, NULL);
}

extern "C" int render_shading_pass_encoded(application_t* app, void* out_radiance, void* out_rgb8) {
	if (!out_rgb8) {
		printf("render_shading_pass_encoded() needs a target for the encoded pixels.\n");
		return 1;
	}
	return render_pass(app, out_radiance, out_rgb8);
}
