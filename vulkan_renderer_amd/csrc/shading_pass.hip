// The frame pipeline behind the reference's entry points (create_shading_pass src/main.c:598, write_constants :2114,
// the vkCmdDraw of record_render_frame_commands :1428-1434): variant selection, constant upload, frame plan, band
// steps, read-back ordering, timing, and the diagnostics that read the pipeline's private buffers (wavefront_kernels.h and
// light_shafts.h define non-template kernels: one unit alone may include them).  The rest of the pass: pass_internal.h.
#include "wavefront_kernels.h"
#include "light_shafts.h"
#include "shade_launchers.h"
#include "pass_internal.h"

using namespace vkr;

// [arithmetic_mode_t + 3 * light textures][strategy]
#define VKR_LAUNCHER_ROW(mode) {vkr_launch_shade_##mode##_0, vkr_launch_shade_##mode##_1, vkr_launch_shade_##mode##_2, vkr_launch_shade_##mode##_3, vkr_launch_shade_##mode##_4}
static const launch_function_t g_launchers[6][5] = {
	VKR_LAUNCHER_ROW(libm), VKR_LAUNCHER_ROW(fast), VKR_LAUNCHER_ROW(exact),
	VKR_LAUNCHER_ROW(textured_libm), VKR_LAUNCHER_ROW(textured_fast), VKR_LAUNCHER_ROW(textured_exact),
};
// [arithmetic_mode_t][strategy - kStrategySeparately]: the kernels with kept prepared polygons; none in the fast mode
#define VKR_PREPARED_ROW(mode) {vkr_launch_shade_prepared_##mode##_2, vkr_launch_shade_prepared_##mode##_3, vkr_launch_shade_prepared_##mode##_4}
static const prepared_launch_function_t g_prepared_launchers[3][3] = {VKR_PREPARED_ROW(libm), {NULL, NULL, NULL}, VKR_PREPARED_ROW(exact)};
static const sector_terms_launch_function_t g_sector_terms_launchers[3] = {vkr_launch_sector_terms_libm, NULL, vkr_launch_sector_terms_exact};
static const error_launch_function_t g_error_launchers[3] = VKR_MODE_LAUNCHERS(vkr_launch_error_display);
static const resolve_launch_function_t g_resolve_launchers[3] = VKR_MODE_LAUNCHERS(vkr_launch_resolve_materials);

// Events that order streams of one device: a device-scope release is all they need.  The default
// (system-scope fence: L2 write-back and invalidation at every record) is paid by whatever runs
// next on the device, and a frame records several.
constexpr unsigned kSyncEventFlags = hipEventDisableTiming | hipEventReleaseToDevice;

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

// the techniques whose samples aim at the light polygon itself: every shadow ray lies inside the light's shaft
static bool aims_at_light_polygon(int technique) {
	return technique == kTechniquePsa || technique == kTechniquePsaBiased || technique == kTechniqueSolidAngle || technique == kTechniqueClippedSolidAngle;
}

// ---- shading pass ----------------------------------------------------------------

// events of a timed frame: its start, the start and the end of the (last band's) shading kernel, its end
constexpr uint32_t kTimingFrameStart = 0, kTimingShadingStart = 1, kTimingShadingEnd = 2, kTimingFrameEnd = 3, kTimingEvents = 4;

static hipEvent_t timing_event(const shading_pass_t* pass, uint32_t slot, uint32_t which) { return ((hipEvent_t*) pass->timing_ring)[kTimingEvents * slot + which]; }

// Buffers of the wavefront ray path, sized for the worst case (every sample of every
// light on every pixel produces a term and a ray) and owned by the pass.
struct wavefront_buffers {
	uint8_t* codes;
	float* terms_visible;
	float* terms_hidden;
	float4* base_color;
	float4* ray_directions;
	uint32_t* ray_records;
	float4* ray_origins;
	uint32_t* ray_queue_size;  // kRayCounterCount live counters (queue sizes, per-XCD work cursors), then last frame's copy
	uint32_t thread_count, max_terms, max_codes, queue_capacity, thread_bits;
	// the streams that only some settings need are allocated when they first do: values of blocked
	// terms (only the plain optimal MIS heuristic has non-zero ones), colour before the sampled terms
	// (only the light display has one); their element counts, 0 while they do not exist
	size_t hidden_term_count, base_color_count;
	// stack entries beyond the LDS part of trace_shadow_rays_wide, [entry][thread of the trace grid];
	// allocated only for trees that can need them
	uint32_t* spill;
	size_t spill_entries;
	// light shafts (light_shafts.h): one word per shading workgroup and light, 1 = no ray of that patch toward that
	// light can be blocked; allocated when the feature first runs
	uint32_t* shaft_clear;
	// what the verdicts in shaft_clear (and the lists in shaft_lists) were derived from: a byte image of the inputs of the
	// most recent launch with these buffers (shaft_arrangement below), shaft_seen_size bytes of it; 0: the tables hold nothing
	// to lean on.  The shaft kernel keeps a verdict only while these bytes are the next launch's, too.
	uint8_t* shaft_seen;
	size_t shaft_seen_size, shaft_seen_capacity;
	size_t shaft_words;
	// ... and per light the plane-space rectangle that the shading kernel tests its rays against
	float4* shaft_rectangles;
	size_t shaft_rectangle_count;
	// ... and per pair kShaftListMax triangle slots: the occluder lists (VKR_SHAFT_LISTS)
	float* shaft_lists;
	size_t shaft_list_words;
	// the second polygon table of every shading workgroup, for the kernel variants that keep one table in LDS only
	// (shading_kernel.h psa_table_in_memory); allocated when such a variant first runs
	float2* psa_table_memory;
	size_t psa_table_bytes;
};

static void free_wavefront_buffers(wavefront_buffers* w) {
	(void) hipFree(w->codes); (void) hipFree(w->terms_visible); (void) hipFree(w->terms_hidden);
	(void) hipFree(w->base_color); (void) hipFree(w->ray_directions); (void) hipFree(w->ray_records); (void) hipFree(w->ray_origins); (void) hipFree(w->ray_queue_size);
	(void) hipFree(w->spill);
	(void) hipFree(w->shaft_clear);
	(void) hipFree(w->shaft_rectangles);
	(void) hipFree(w->shaft_lists);
	free(w->shaft_seen);
	(void) hipFree(w->psa_table_memory);
	memset(w, 0, sizeof(*w));
}

// The prepared polygons of the most recent launches (shading_kernel.h "Prepared polygons that are still true")
enum { kCacheEmpty = 0, kCachePending = 1, kCacheValid = 2 };
struct prepared_cache {
	uint4* buffer;  // the second argument of the storing and the loading kernel, allocated when a launch first stores
	size_t buffer_quads;
	// the sector terms of the polygons in `buffer` (shading_kernel.h "Sector terms that are still true"): the third argument of
	// the kernel that loads with terms, allocated, retained and released by the rules of `buffer`, and filled behind the storing
	// launch, in front of `stored`.  terms_quads: its size, 0: the launches of this arrangement load without terms
	float4* terms;
	size_t terms_quads;
	// a byte image of everything the preparation reads (prepared_arrangement below), of the most recent launch that the
	// cache could serve: seen_size bytes, 0: none
	uint8_t* seen;
	size_t seen_size, seen_capacity;
	uint8_t* scratch;
	size_t scratch_capacity;
	// kCachePending: a storing launch with the inputs in `seen` has been submitted and `stored` recorded behind it;
	// kCacheValid: that event has been seen complete - launches with these inputs load
	uint32_t state;
	hipEvent_t stored;
	hipStream_t stored_stream;  // the stream of that storing launch
	// VKR_PREPARED_POLYGONS_MIB: the largest buffer that is allocated (0: no launch stores or loads)
	uint32_t budget_mib;
	// for get_prepared_polygon_statistics(): the mode of the last launch, launches per mode, launches that ran plain because
	// the storing launch had not completed yet
	uint32_t last_mode;
	uint64_t launches[3], waited;
	// VKR_SECTOR_TERMS=0: no terms are kept; for get_sector_terms_statistics(): loading launches with and without terms
	uint32_t terms_enabled;
	uint64_t loaded_with_terms, loaded_without_terms;
};

// What a frame in flight owns.  With frames_in_flight = n >= 2 consecutive frames take turns
// on n contexts (and n of the device's frame streams); otherwise only context 0 is used, on
// device->stream.
struct frame_context {
	wavefront_buffers buffers;
	hipEvent_t done;  // recorded behind the last kernel of the frame
	bool recorded;    // `done` has been recorded: the next frame's resolve is ordered behind it
	// what the context's most recent launches wrote their output to (a ring of the last eight): a launch only has to be ordered
	// behind another one when they write the same buffer (frames of a slab exchange take turns on several slabs, round 6); the
	// context's `done` event lies behind all of them
	const void* targets[8];
	uint32_t target_cursor;
	bool pending;     // device->stream has not been made to wait for `done` yet
	uint32_t readers_seen;  // frame_pipeline::readers_generation this context's stream has waited for
};
struct frame_pipeline {
	frame_context contexts[VKR_MAX_FRAMES_IN_FLIGHT];
	hipEvent_t inputs_ready;  // marks what device->stream had submitted when a frame started
	// Recorded on device->stream behind every kernel there that reads a target of the frames
	// (output encoding of the frame or of a slab): a later frame in flight must not resolve into
	// that target before the reader is done.  (finish_frames() orders device->stream behind the
	// frames; this is the opposite direction.)
	hipEvent_t readers_done;
	uint32_t readers_generation;
	// bumped whenever an input that the frames read from device memory has been rewritten (visibility buffer, scene):
	// part of what the light shafts' verdicts are derived from (shaft_arrangement)
	uint32_t inputs_generation;
	// where run_light_shafts() puts the inputs of a launch together before it compares them with the context's copy
	uint8_t* shaft_scratch;
	size_t shaft_scratch_capacity;
	// the polygon tables in device memory (wavefront_buffers::psa_table_memory) of the frames without wavefront rays, which
	// own no context
	wavefront_buffers device_stream_buffers;
	// the prepared polygons that the shading kernel keeps while its inputs stand still ("prepared polygon cache" below): one
	// per pass, not per frame context - it is read-only while it is valid
	prepared_cache prepared;
	uint32_t next;            // context of the next pipelined frame
	uint32_t last;            // context of the most recent frame
	uint32_t depth;           // frames in flight of the most recent pipelined frame
	// tuning / test knobs, read from the environment once when the pipeline is created:
	// VKR_WIDE_STACK_LDS (stack entries per lane that trace_shadow_rays_wide keeps in LDS: tests shrink
	// it to drive rays through the spill path)
	// VKR_WAVEFRONT_BUDGET_MIB: most device memory that all sets of wavefront buffers in flight may take
	// (default 36864 - config 4 then runs as three bands of 12 GB, the fastest of 1 ... 12 bands, profiles/r04c/: a
	// frame whose worst case needs more is rendered in bands); VKR_BAND_COUNT forces
	// the number of bands per frame (0: automatic)
	// VKR_LIGHT_SHAFTS: 0 turns the shaft test off (every shadow ray is traced, as until round 3), 1 on; default 2:
	// on when a pixel may queue 8 rays or more (samples x techniques x lights) - the walk of a patch costs about as
	// much as tracing 2.5 rays per pixel and light, and it is the patches with many rays per light and several lights
	// that repay it (measured, profiles/r05m: config 3, 32 rays per pixel, 1.553 -> 1.443 ms; config 4, 128, 25.9 -> 23.0;
	// the target shape, 8, 0.488 -> 0.500 before the occluder lists and 0.501 -> 0.443 with them, which is what moved
	// the rule from 16 to 8; config 2, 2 rays per pixel, 0.127 -> 0.192)
	// VKR_SHAFT_REST, VKR_SHAFT_MAX_STEPS, VKR_WIDE_REFILL, VKR_WIDE_REFILL_BELOW (round 5): ensure_frames()
	uint32_t wide_stack_lds, wide_refill, wide_refill_below, wavefront_budget_mib, band_count, light_shafts, shaft_lists, shaft_rest, shaft_max_steps;
};

static uint32_t environment_knob(const char* name, uint32_t fallback, uint32_t low, uint32_t high) {
	const char* text = getenv(name);
	if (!text || !text[0]) return fallback;
	long value = strtol(text, NULL, 10);
	return (uint32_t) (value < (long) low ? (long) low : (value > (long) high ? (long) high : value));
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
	free(frames->shaft_scratch);
	(void) hipFree(frames->prepared.buffer);
	(void) hipFree(frames->prepared.terms);
	if (frames->prepared.stored) (void) hipEventDestroy(frames->prepared.stored);
	free(frames->prepared.seen);
	free(frames->prepared.scratch);
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
		|| hipEventCreateWithFlags(&frames->prepared.stored, kSyncEventFlags) != hipSuccess;
	for (int i = 0; i != VKR_MAX_FRAMES_IN_FLIGHT && !failed; ++i) failed = hipEventCreateWithFlags(&frames->contexts[i].done, kSyncEventFlags) != hipSuccess;
	if (failed) {
		printf("Failed to create the events of the frame pipeline.\n");
		destroy_wavefront(pass);
		return NULL;
	}
	frames->wide_stack_lds = environment_knob("VKR_WIDE_STACK_LDS", kWideStackLds, 4u, kWideStackLds);
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
	// VKR_WIDE_REFILL: lanes of a tracing wave (four-wide tree) that have to be idle before they are handed the next rays,
	// once the wave has found its batches less than VKR_WIDE_REFILL_BELOW / 256 busy (wavefront_kernels.h; 256: from the
	// first batch on); 0: a batch of 64 rays is always walked to its end first (until round 4)
	frames->wide_refill = environment_knob("VKR_WIDE_REFILL", kWideRefillLanes, 0u, 64u);
	frames->wide_refill_below = environment_knob("VKR_WIDE_REFILL_BELOW", kWideRefillBelow, 0u, 256u);
	frames->wavefront_budget_mib = environment_knob("VKR_WAVEFRONT_BUDGET_MIB", 36864u, 64u, 262144u);
	frames->band_count = environment_knob("VKR_BAND_COUNT", 0u, 0u, 4096u);
	// VKR_PREPARED_POLYGONS_MIB: most device memory that the kept prepared polygons of a launch may take; 0: nothing is kept,
	// every launch prepares its polygons itself.  (Config 3 at 1920x1080 keeps 2 040 MiB: 2.09 M threads x 4 lights x 256 B.)
	// (with the sector terms of those polygons - as much again at V = 5 - where both fit: 4 080 MiB)
	frames->prepared.budget_mib = environment_knob("VKR_PREPARED_POLYGONS_MIB", 4096u, 0u, 262144u);
	// VKR_SECTOR_TERMS=0: the loading launches compute the terms of their sectors themselves
	frames->prepared.terms_enabled = environment_knob("VKR_SECTOR_TERMS", 1u, 0u, 1u);
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

// host memory that grows on demand and keeps its content
static int grow_bytes(uint8_t** buffer, size_t* capacity, size_t size) {
	if (*capacity >= size) return 0;
	uint8_t* grown = (uint8_t*) realloc(*buffer, size);
	if (!grown) return 1;
	*buffer = grown;
	*capacity = size;
	return 0;
}

// The same for a device buffer of `count` elements, whose content is not kept: a buffer that is too small is freed
// (while other frames may be in flight: hipFree waits for the device) and allocated anew.  On failure pointer and count
// are zero and `message` is printed, a format for the MiB that were asked for.
template <typename T>
static int grow_device_buffer(T** buffer, size_t* count, size_t wanted, size_t element_bytes, const char* message) {
	if (wanted <= *count) return 0;
	(void) hipFree(*buffer);
	*buffer = NULL; *count = 0;
	if (hipMalloc(buffer, wanted * element_bytes) != hipSuccess) {
		printf(message, wanted * element_bytes / 1048576.0);
		return 1;
	}
	*count = wanted;
	return 0;
}

static int ensure_shaft_words(wavefront_buffers* w, size_t words, uint32_t light_count, bool lists, hipStream_t stream) {
	size_t list_words = lists ? words * kShaftListMax * kShaftListEntry : 0;
	const bool fresh_words = words > w->shaft_words;
	// (the tables carry state from frame to frame: whichever of them is allocated anew, the copy of the inputs is forgotten)
	if (list_words > w->shaft_list_words || light_count > w->shaft_rectangle_count || fresh_words) w->shaft_seen_size = 0;
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
	// the record word of a ray: thread and code cursor (shading_kernel.h ray_record)
	uint32_t thread_bits = 1;
	while (thread_bits < 32 && (1ull << thread_bits) < thread_count) ++thread_bits;
	if (terms >= 0xFFFFFFFFull || (size_t) (max_codes + 3u) * thread_count >= 0xFFFFFFFFull || thread_bits >= 32 || ((uint64_t) max_codes << thread_bits) > 0xFFFFFFFFull) {
		printf("The wavefront ray queue would need more than 2^32 entries (%u threads x %u terms); render in more bands or use inline rays.\n", thread_count, max_terms);
		return 1;
	}
	w->thread_bits = thread_bits;
	w->queue_capacity = queue_capacity_for(thread_count, max_terms);
	size_t ray_slots = (size_t) w->queue_capacity * kRayQueueCount;
	// (codes are stored four to a word per thread: code_slot() in shading_kernel.h)
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

void note_target_reader(application_t* app) {
	frame_pipeline* frames = (frame_pipeline*) app->shading_pass.wavefront;
	if (!frames || !app->shading_pass.last_frame_in_flight) return;
	if (hipEventRecord(frames->readers_done, (hipStream_t) app->device.stream) == hipSuccess) ++frames->readers_generation;
}

// The constant buffer is a small ring: the host may record several frames ahead, so
// every set of constants in flight needs its own staging and device copy (the reference
// keeps one uniform buffer per swapchain image for the same reason, main.c:330-360).
// A frame whose constants are byte-identical to the previous frame's reuses the slot
// that is already on the device (static camera and lights: no upload at all, like the
// reference's host-coherent uniform buffer, which costs no GPU time either).
constexpr uint32_t kConstantSlots = VKR_MAX_FRAMES_IN_FLIGHT + 2;
// (device->stream and the frame streams)
constexpr int kConstantReaders = 1 + VKR_MAX_FRAMES_IN_FLIGHT;
struct constants_ring {
	void* host[kConstantSlots];
	void* device[kConstantSlots];
	// a slot may be read from device->stream and from the frame streams
	hipEvent_t consumed[kConstantSlots][kConstantReaders];
	hipEvent_t uploaded[kConstantSlots];
	// bit i: readers[i] (device->stream, then the frame streams) is ordered behind the upload
	uint32_t ordered[kConstantSlots];
	bool in_flight[kConstantSlots];
	void* scratch;    // write_constants target before it is known whether anything changed
	uint32_t current; // slot whose device copy the next launch reads
	bool valid;       // false until the first upload
};

static void destroy_constants_ring(shading_pass_t* pass, const device_t* device) {
	constants_ring* ring = (constants_ring*) pass->constants_ring;
	if (!ring) return;
	for (uint32_t i = 0; i != kConstantSlots; ++i) {
		vkr_device_free(ring->device[i], device);
		vkr_host_free_pinned(ring->host[i]);
		for (hipEvent_t event : ring->consumed[i]) if (event) (void) hipEventDestroy(event);
		if (ring->uploaded[i]) (void) hipEventDestroy(ring->uploaded[i]);
	}
	free(ring->scratch);
	free(ring);
	pass->constants_ring = NULL;
	pass->constants_device = pass->constants_host = NULL;
}

static int create_constants_ring(shading_pass_t* pass, const device_t* device) {
	constants_ring* ring = (constants_ring*) calloc(1, sizeof(constants_ring));
	pass->constants_ring = ring;
	if (!ring) return 1;
	ring->scratch = calloc(1, pass->constants_size);
	if (!ring->scratch) return 1;
	for (uint32_t i = 0; i != kConstantSlots; ++i) {
		if (vkr_device_alloc(&ring->device[i], device, pass->constants_size, "the constant buffer")
			|| vkr_host_alloc_pinned(&ring->host[i], pass->constants_size)
			|| hip_failed(hipEventCreateWithFlags(&ring->uploaded[i], kSyncEventFlags), "creating upload events"))
			return 1;
		for (hipEvent_t& event : ring->consumed[i])
			if (hip_failed(hipEventCreateWithFlags(&event, kSyncEventFlags), "creating upload events")) return 1;
		memset(ring->host[i], 0, pass->constants_size);
	}
	pass->constants_device = ring->device[0];
	pass->constants_host = ring->host[0];
	return 0;
}

int upload_constants(application_t* app, hipStream_t stream) {
	shading_pass_t* pass = &app->shading_pass;
	constants_ring* ring = (constants_ring*) pass->constants_ring;
	// a frame stream that does not exist yet is marked by `present`: a NULL stream is a stream too
	hipStream_t readers[kConstantReaders] = {(hipStream_t) app->device.stream};
	bool present[kConstantReaders] = {true};
	for (int i = 0; i != VKR_MAX_FRAMES_IN_FLIGHT; ++i) {
		readers[1 + i] = (hipStream_t) app->device.frame_streams[i];
		present[1 + i] = app->device.frame_streams[i] != NULL;
	}
	write_constants(ring->scratch, app);
	if (!ring->valid || memcmp(ring->scratch, ring->host[ring->current], pass->constants_size) != 0) {
		uint32_t slot = ring->valid ? (ring->current + 1) % kConstantSlots : 0;
		// everything launched so far may read the old slot: it is free again once all
		// streams have passed this point
		if (ring->valid) {
			// (an absent reader's event stays unrecorded, which completes at once)
			for (int i = 0; i != kConstantReaders; ++i) if (present[i]) (void) hipEventRecord(ring->consumed[ring->current][i], readers[i]);
			ring->in_flight[ring->current] = true;
		}
		if (ring->in_flight[slot])
			for (int i = 0; i != kConstantReaders; ++i)
				if (hip_failed(hipEventSynchronize(ring->consumed[slot][i]), "waiting for a free constant buffer")) return 1;
		ring->in_flight[slot] = false;
		memcpy(ring->host[slot], ring->scratch, pass->constants_size);
		if (hip_failed(hipMemcpyAsync(ring->device[slot], ring->host[slot], pass->constants_size, hipMemcpyHostToDevice, stream), "uploading the constants")
			|| hip_failed(hipEventRecord(ring->uploaded[slot], stream), "recording the upload"))
			return 1;
		ring->ordered[slot] = 0;
		for (int i = 0; i != kConstantReaders; ++i) if (present[i] && readers[i] == stream) ring->ordered[slot] |= 1u << i;
		ring->current = slot;
		ring->valid = true;
		pass->constants_device = ring->device[slot];
		pass->constants_host = ring->host[slot];
		return 0;
	}
	// unchanged constants that another stream uploaded: order this stream behind that upload
	for (int i = 0; i != kConstantReaders; ++i)
		if (present[i] && readers[i] == stream) {
			if (ring->ordered[ring->current] & (1u << i)) return 0;
			ring->ordered[ring->current] |= 1u << i;
		}
	return hip_failed(hipStreamWaitEvent(stream, ring->uploaded[ring->current], 0), "waiting for the constants");
}

// ---- asynchronous read-back through pinned staging (include/vkr_shading_pass.h begin_read_back) ----------------
// One staging buffer, one event and the device address it was filled from per slot; all copies run on one stream of their
// own (device-to-host copies into pinned memory are served by a DMA engine: they take no compute unit from the frames).
constexpr uint32_t kReadBackSlots = VKR_MAX_FRAMES_IN_FLIGHT + 1;
struct read_back_state {
	hipStream_t stream;
	hipEvent_t source_ready;               // marks device->stream when a copy is queued
	void* staging[kReadBackSlots];
	size_t staging_size[kReadBackSlots];
	hipEvent_t copied[kReadBackSlots];
	const void* source[kReadBackSlots];    // device range [source, source + bytes) of the slot's most recent copy
	size_t bytes[kReadBackSlots];
	bool pending[kReadBackSlots];          // the copy may still be running: a writer of its source waits for `copied`
	// readers outside the pass (vkr_note_target_reader: the slab exchange's collectives): an event of the caller and the
	// device range that is read until it completes
	hipEvent_t reader_event[kReadBackSlots];
	const void* reader_source[kReadBackSlots];
	size_t reader_bytes[kReadBackSlots];
};

// ... and before the caller destroys such an event
extern "C" void vkr_forget_target_reader(application_t* app, void* event) {
	read_back_state* rb = (read_back_state*) app->shading_pass.readback;
	if (!rb || !event) return;
	for (uint32_t i = 0; i != kReadBackSlots; ++i)
		if (rb->reader_event[i] == (hipEvent_t) event) rb->reader_event[i] = NULL;
	if (app->shading_pass.wait_before_next_frame == event) app->shading_pass.wait_before_next_frame = NULL;
}

static read_back_state* ensure_read_back_state(shading_pass_t* pass) {
	if (!pass->readback) pass->readback = calloc(1, sizeof(read_back_state));
	return (read_back_state*) pass->readback;
}

// For host/slab_exchange.c: `event` (a hipEvent_t of the caller, recorded behind a reader of [target, target + bytes)) must
// have completed before a later frame writes that range.  The frame that writes it waits on the device, in front of the
// kernel that does the writing - the resolve kernel of a frame with wavefront rays, the shading kernel otherwise, the
// encoding kernel for an encoded slab - and not in front of its first kernel, as shading_pass_t.wait_before_next_frame
// makes it: shaft walks, shading and tracing of frame k + n overlap the collective of frame k (round 6: a rank's slab at
// N = 8 took 0.220 instead of 0.176 ms through the exchange with a collective that did nothing,
// profiles/r10c/exchange_overhead_before.jsonl).  One entry per range; a new event for a known range replaces the old one.
extern "C" void vkr_note_target_reader(application_t* app, void* event, const void* target, size_t bytes) {
	read_back_state* rb = ensure_read_back_state(&app->shading_pass);
	if (!rb) return;
	uint32_t slot = kReadBackSlots;
	for (uint32_t i = 0; i != kReadBackSlots; ++i) {
		if (rb->reader_event[i] && rb->reader_source[i] == target) { slot = i; break; }
		if (!rb->reader_event[i] && slot == kReadBackSlots) slot = i;
	}
	if (slot == kReadBackSlots) {
		// (more ranges than buffer sets can exist: fall back to the oldest rule - the whole next frame waits)
		app->shading_pass.wait_before_next_frame = event;
		return;
	}
	rb->reader_event[slot] = (hipEvent_t) event;
	rb->reader_source[slot] = target;
	rb->reader_bytes[slot] = bytes;
}

static void destroy_read_back(shading_pass_t* pass) {
	read_back_state* rb = (read_back_state*) pass->readback;
	if (!rb) return;
	if (rb->stream) { (void) hipStreamSynchronize(rb->stream); (void) hipStreamDestroy(rb->stream); }
	if (rb->source_ready) (void) hipEventDestroy(rb->source_ready);
	for (uint32_t i = 0; i != kReadBackSlots; ++i) {
		if (rb->copied[i]) (void) hipEventDestroy(rb->copied[i]);
		vkr_host_free_pinned(rb->staging[i]);
	}
	free(rb);
	pass->readback = NULL;
}

// Makes `stream` wait for every pending copy that reads from [target, target + bytes): called in front of the kernel
// of a frame that writes its output (the resolve kernel with wavefront rays, the shading kernel otherwise)
static void wait_for_read_backs_of(shading_pass_t* pass, const void* target, size_t bytes, hipStream_t stream) {
	read_back_state* rb = (read_back_state*) pass->readback;
	if (!rb) return;
	for (uint32_t i = 0; i != kReadBackSlots; ++i) {
		if (!rb->reader_event[i]) continue;
		const uint8_t* a = (const uint8_t*) rb->reader_source[i];
		const uint8_t* b = (const uint8_t*) target;
		if (!(a < b + bytes && b < a + rb->reader_bytes[i])) continue;
		if (hipEventQuery(rb->reader_event[i]) == hipSuccess) { rb->reader_event[i] = NULL; continue; }
		(void) hipStreamWaitEvent(stream, rb->reader_event[i], 0);
	}
	for (uint32_t i = 0; i != kReadBackSlots; ++i) {
		if (!rb->pending[i]) continue;
		if (hipEventQuery(rb->copied[i]) == hipSuccess) { rb->pending[i] = false; continue; }
		const uint8_t* a = (const uint8_t*) rb->source[i];
		const uint8_t* b = (const uint8_t*) target;
		if (a < b + bytes && b < a + rb->bytes[i]) (void) hipStreamWaitEvent(stream, rb->copied[i], 0);
	}
}

// For csrc/frame_statistics.hip, whose kernels read and write targets on streams of their own
extern "C" void vkr_order_target_write(application_t* app, const void* target, size_t bytes, void* stream) {
	wait_for_read_backs_of(&app->shading_pass, target, bytes, (hipStream_t) stream);
}

// Makes `stream` wait for the frames in flight: the most recent frame of every context (earlier frames of a context precede
// it on the context's stream).  begin_read_back() waits for the most recent frame only, which covers the one buffer that
// frame wrote; a reader of several frames' targets - an accumulation of a ring - needs them all, and frames that wrote
// different targets do not wait for each other.
extern "C" int vkr_order_behind_frames_in_flight(application_t* app, void* stream) {
	frame_pipeline* frames = (frame_pipeline*) app->shading_pass.wavefront;
	if (!frames || !app->shading_pass.last_frame_in_flight) return 0;
	for (frame_context& c : frames->contexts)
		if (c.recorded && hip_failed(hipStreamWaitEvent((hipStream_t) stream, c.done, 0), "ordering a reader behind the frames in flight")) return 1;
	return 0;
}

extern "C" int begin_read_back(application_t* app, uint32_t slot, const void* device_source, uint64_t bytes) {
	shading_pass_t* pass = &app->shading_pass;
	if (slot >= kReadBackSlots) {
		printf("begin_read_back(): slot %u does not exist (0 ... %u).\n", slot, kReadBackSlots - 1u);
		return 1;
	}
	if (!device_source) {
		device_source = app->render_targets.radiance;
		bytes = sizeof(float) * 4 * (uint64_t) app->swapchain.extent.width * app->swapchain.extent.height;
	}
	if (!device_source || !bytes) {
		printf("begin_read_back() needs a device buffer (or render targets) to read from.\n");
		return 1;
	}
	read_back_state* rb = ensure_read_back_state(pass);
	if (!rb) return 1;
	if (!rb->stream && (hip_failed(hipStreamCreateWithFlags(&rb->stream, hipStreamNonBlocking), "creating the read-back stream")
		|| hip_failed(hipEventCreateWithFlags(&rb->source_ready, kSyncEventFlags), "creating read-back events")))
		return 1;
	// (the host waits for this one: no device-scope-only release)
	if (!rb->copied[slot] && hip_failed(hipEventCreateWithFlags(&rb->copied[slot], hipEventDisableTiming), "creating read-back events")) return 1;
	// (the slot's previous copy has to have landed before its staging memory is reused or freed)
	if (rb->pending[slot] && hip_failed(hipEventSynchronize(rb->copied[slot]), "waiting for the slot's previous read-back")) return 1;
	rb->pending[slot] = false;
	if (rb->staging_size[slot] < bytes) {
		vkr_host_free_pinned(rb->staging[slot]);
		rb->staging[slot] = NULL; rb->staging_size[slot] = 0;
		if (vkr_host_alloc_pinned(&rb->staging[slot], (size_t) bytes)) {
			printf("Failed to allocate %.1f MiB of pinned host memory for read-backs.\n", bytes / 1048576.0);
			return 1;
		}
		rb->staging_size[slot] = (size_t) bytes;
	}
	// behind the most recent frame in flight (only that one: its resolves wait for earlier frames that wrote the same target,
	// not for those that wrote another one, which may still be running) ...
	frame_pipeline* frames = (frame_pipeline*) pass->wavefront;
	if (frames && pass->last_frame_in_flight) {
		frame_context* last = &frames->contexts[frames->last];
		if (last->recorded && hip_failed(hipStreamWaitEvent(rb->stream, last->done, 0), "ordering the read-back behind the frame")) return 1;
	}
	// ... and behind what device->stream has queued (frames without the pipeline, output encoding, an assembled frame)
	if (hip_failed(hipEventRecord(rb->source_ready, (hipStream_t) app->device.stream), "marking the source")
		|| hip_failed(hipStreamWaitEvent(rb->stream, rb->source_ready, 0), "ordering the read-back behind the device stream")
		|| hip_failed(hipMemcpyAsync(rb->staging[slot], device_source, (size_t) bytes, hipMemcpyDeviceToHost, rb->stream), "queueing the read-back")
		|| hip_failed(hipEventRecord(rb->copied[slot], rb->stream), "marking the read-back"))
		return 1;
	rb->source[slot] = device_source;
	rb->bytes[slot] = (size_t) bytes;
	rb->pending[slot] = true;
	return 0;
}

extern "C" const void* end_read_back(application_t* app, uint32_t slot) {
	read_back_state* rb = (read_back_state*) app->shading_pass.readback;
	if (!rb || slot >= kReadBackSlots || !rb->staging[slot] || !rb->copied[slot]) {
		printf("end_read_back(): slot %u has no read-back in flight.\n", slot);
		return NULL;
	}
	if (hip_failed(hipEventSynchronize(rb->copied[slot]), "waiting for the read-back")) return NULL;
	rb->pending[slot] = false;
	return rb->staging[slot];
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

// What render_pass() decides about a frame before its first band (plan_frame, plan_bands); the band steps read it
struct frame_plan {
	shade_params p;          // the parameters of every launch of the frame; a band step adds the band's blocks and buffers
	frame_pipeline* frames;  // NULL for a frame without wavefront rays, unless its polygon tables live in device memory
	int strategy, technique, capacity, error_mode, ray_mode;
	// how the launch gets its prepared polygons (kPreparedPlain / kPreparedStoring / kPreparedLoading, choose_prepared_mode()) and
	// the buffer of the other two than plain
	int prepared_mode;
	uint4* prepared;
	// quads (16 B) of the buffer that the prepared polygons of the frame's one launch may take: plan_bands() has found room for
	// them in the budgets; 0: this frame keeps none
	size_t prepared_quads;
	// ... and the sector terms of those polygons: the buffer of the kernel that loads with terms, and its quads - 0: the budgets
	// hold the polygons alone (or VKR_SECTOR_TERMS=0), and the launches load without terms
	const float4* terms;
	size_t terms_quads;
	// (table_in_memory: the kernel variants that keep one of their two polygon tables in device memory, shading_kernel.h psa_table_in_memory)
	bool table_in_memory, hidden_terms, base_color, use_wide_tree, textured, pipelined;
	uint32_t grid_blocks, table_bytes_per_workgroup, max_terms;
	// frames in flight (1: not pipelined), the bands of the frame, workgroups of the tracing kernels (wavefront rays only)
	uint32_t depth, band_count, blocks_per_band, trace_blocks;
	// bytes of the output this call writes (a slab in slab layout, else the frame): what pending read-backs are checked against
	size_t frame_output_bytes;
};

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

// Which launches can keep prepared polygons at all ("prepared polygon cache" below): the kernel variants of
// prepared_polygons_apply() (shading_kernel.h), untextured.  plan_bands() adds: one launch per frame, and room in the budgets.
static bool prepared_polygons_possible(const application_t* app, const frame_plan* f) {
	return f->ray_mode == kRaysDeferredBlocks && f->error_mode == kErrorNone && !f->table_in_memory && !f->textured
		&& !f->p.light_texture_descriptors && app->shading_pass.arithmetic_mode != arithmetic_mode_fast && f->p.light_count != 0
		&& (f->technique == kTechniquePsa || f->technique == kTechniquePsaBiased) && f->strategy >= kStrategySeparately && f->strategy <= kStrategyRandom
		&& f->capacity >= 4 && f->capacity <= 5;
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
	// The prepared polygons of a frame that is one launch (a frame in bands meets a context's buffers with another band each
	// time, and config 4, the frame that is rendered in bands, has no such kernel variant): one buffer per pass, counted against
	// the budget of the wavefront buffers like the shafts' tables, and against VKR_PREPARED_POLYGONS_MIB.  (bind_textures() runs
	// after this: a frame with light textures is turned away by choose_prepared_mode().)
	f->prepared_quads = f->terms_quads = 0;
	if (f->band_count == 1 && frames->prepared.budget_mib != 0u && prepared_polygons_possible(app, f)) {
		const uint32_t thread_count = f->blocks_per_band * 256u;
		const size_t quads = (size_t) thread_count * f->p.light_count * (prepared_bytes_per_pair(f->capacity) / 16u);
		const double bytes = 16.0 * (double) quads;
		if (bytes <= (double) frames->prepared.budget_mib * 1048576.0
			&& f->depth * wavefront_bytes(thread_count, f->max_terms, f->p.light_count, f->hidden_terms, f->base_color, 0u) + bytes <= budget)
			f->prepared_quads = quads;
		// the terms count against both budgets together with the polygons; where only the polygons fit, the launch loads without
		const size_t terms_quads = (size_t) thread_count * f->p.light_count * (sector_terms_bytes_per_pair(f->capacity) / 16u);
		const double both = bytes + 16.0 * (double) terms_quads;
		if (f->prepared_quads != 0 && frames->prepared.terms_enabled && both <= (double) frames->prepared.budget_mib * 1048576.0
			&& f->depth * wavefront_bytes(thread_count, f->max_terms, f->p.light_count, f->hidden_terms, f->base_color, 0u) + both <= budget)
			f->terms_quads = terms_quads;
	}
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
		// a region per workgroup of the launch, in the launch's own buffers (shading_kernel.h psa_table_in_memory)
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

// What the verdicts of a launch are derived from, as bytes (light_shafts.h "Verdicts that are still true"): a frame context
// keeps the image of its most recent launch (wavefront_buffers::shaft_seen) and the next launch is compared with it by
// memcmp - exactly, not through a hash: "the same" now keeps a "clear" or a list, and a collision would keep a wrong one.
// The image has two parts.  The ARRANGEMENT is this struct and, behind it, the ranges of the constants that the shading
// positions are computed from (the camera's, the mesh's de-quantisation); then comes one record per LIGHT, its bytes in
// the constants.
// Who changes an input and how that shows here: a BVH build (scene load) gives the tree a new build_serial; whoever
// rewrites the visibility buffer or another input in device memory - render_visibility_pass, upload_visibility, a caller
// on its own through mark_inputs_changed() (INTEGRATION.md obliges it to) - bumps inputs_generation; camera, lights and
// the de-quantisation reach the kernels through write_constants() alone, whose bytes are compared themselves.
struct shaft_arrangement {
	uint32_t first_block, block_count, width, height, tile_size, rank, rank_count, tiles_x, tile_count, slab_layout;
	uint32_t light_count, max_light_vertex_count, lists, groups, max_steps;
	uint32_t inputs_generation, build_serial, build_bits, node_count, wide_node_count;
	float extent;
	uint32_t light_stride;
	const void *visibility, *positions, *nodes, *triangles, *wide_nodes;
	float grid_origin[3], grid_inverse_cell[3];
};
static_assert(sizeof(shaft_arrangement) == 22 * 4 + 5 * sizeof(void*) + 6 * 4, "no padding: the struct is compared as bytes");

// Puts the image of this launch's inputs together, compares it with the context's copy and keeps it as the new copy.
// -> arrangement_same, same_lights (bit i: arrangement and light i < 32 are byte-equal to the previous launch's)
static int compare_shaft_inputs(frame_pipeline* frames, wavefront_buffers* w, const shading_pass_t* pass, const shaft_arrangement& arrangement, bool& arrangement_same, uint32_t& same_lights) {
	arrangement_same = false;
	same_lights = 0u;
	const uint8_t* constants = (const uint8_t*) pass->constants_host;
	const size_t ranges[2][2] = {{offsetof(per_frame_constants_t, world_to_projection_space), offsetof(per_frame_constants_t, mis_visibility_estimate)},
		{offsetof(per_frame_constants_t, mesh_dequantization_factor), offsetof(per_frame_constants_t, error_factor)}};
	const size_t light_bytes = (size_t) arrangement.light_stride * arrangement.light_count;
	size_t arrangement_bytes = sizeof(shaft_arrangement);
	for (const size_t* range : ranges) arrangement_bytes += range[1] - range[0];
	const size_t size = arrangement_bytes + light_bytes;
	if (grow_bytes(&frames->shaft_scratch, &frames->shaft_scratch_capacity, size) || grow_bytes(&w->shaft_seen, &w->shaft_seen_capacity, size)) {
		printf("Failed to allocate %zu bytes for the inputs of the light shafts.\n", size);
		w->shaft_seen_size = 0;
		return 1;
	}
	uint8_t* now = frames->shaft_scratch;
	memcpy(now, &arrangement, sizeof(arrangement));
	size_t cursor = sizeof(arrangement);
	for (const size_t* range : ranges) {
		memcpy(now + cursor, constants + range[0], range[1] - range[0]);
		cursor += range[1] - range[0];
	}
	memcpy(now + cursor, constants + sizeof(per_frame_constants_t), light_bytes);
	if (w->shaft_seen_size == size && memcmp(now, w->shaft_seen, arrangement_bytes) == 0) {
		arrangement_same = true;
		for (uint32_t i = 0; i != arrangement.light_count && i != 32u; ++i) {
			const size_t at = arrangement_bytes + (size_t) arrangement.light_stride * i;
			if (memcmp(now + at, w->shaft_seen + at, arrangement.light_stride) == 0) same_lights |= 1u << i;
		}
	}
	memcpy(w->shaft_seen, now, size);
	w->shaft_seen_size = size;
	return 0;
}

// Band step 4: the shaft kernel of the band where light_shafts_apply(), its tables in p
static int run_light_shafts(application_t* app, frame_plan* f, frame_context* frame, hipStream_t stream) {
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
	arrangement.first_block = p.first_block; arrangement.block_count = p.block_count;
	arrangement.width = p.width; arrangement.height = p.height;
	arrangement.tile_size = p.tile_size; arrangement.rank = p.rank; arrangement.rank_count = p.rank_count;
	arrangement.tiles_x = p.tiles_x; arrangement.tile_count = p.tile_count; arrangement.slab_layout = p.slab_layout;
	arrangement.light_count = p.light_count; arrangement.max_light_vertex_count = p.max_light_vertex_count;
	arrangement.lists = lists ? 1u : 0u; arrangement.groups = shaft_groups; arrangement.max_steps = max_steps;
	arrangement.inputs_generation = frames->inputs_generation;
	arrangement.build_serial = structure->build_serial;
	memcpy(&arrangement.build_bits, &structure->build_milliseconds, sizeof(arrangement.build_bits));
	arrangement.node_count = structure->node_count; arrangement.wide_node_count = structure->wide_node_count;
	arrangement.extent = extent;
	arrangement.light_stride = (uint32_t) ((pass->constants_size - sizeof(per_frame_constants_t)) / p.light_count);
	arrangement.visibility = p.visibility; arrangement.positions = p.positions;
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
		frame->buffers.shaft_seen_size = 0;
		return 1;
	}
	p.shaft_clear = frame->buffers.shaft_clear;
	p.shaft_rectangles = frame->buffers.shaft_rectangles;
	p.shaft_lists = lists ? frame->buffers.shaft_lists : NULL;
	pass->last_shaft_groups = shaft_groups;
	return 0;
}

// ---- prepared polygon cache ------------------------------------------------------------------
// Everything the preparation of a launch reads, as bytes: this struct and behind it the constants of the launch - camera,
// de-quantisation, roughness factor, the LTC table's lookup constants and every light's record - with the four noise
// words blanked, which only the samples read.  (The constants hold more than the preparation reads - exposure, the MIS
// visibility estimate: a change of those costs one plain and one storing launch and nothing else.)
// What lies behind the pointers is named by inputs_generation (visibility buffer, mark_inputs_changed()), the tree's
// build_serial (mesh and materials are uploaded with it, load_scene()) and the LTC table's upload_serial.
struct prepared_arrangement {
	uint32_t first_block, block_count, thread_count, width, height, tile_size, rank, rank_count, tiles_x, tile_count, slab_layout;
	uint32_t light_count, max_light_vertex_count, strategy, technique, capacity, arithmetic_mode;
	uint32_t inputs_generation, build_serial, ltc_serial, ltc_resolution, ltc_layer_count;
	const void *visibility, *positions, *normals_and_tex_coords, *material_indices, *material_constants, *ltc_rgba, *ltc_rg;
};
static_assert(sizeof(prepared_arrangement) == 22 * 4 + 7 * sizeof(void*), "no padding: the struct is compared as bytes");

static void forget_prepared_polygons(frame_pipeline* frames) {
	if (!frames) return;
	frames->prepared.state = kCacheEmpty;
	frames->prepared.seen_size = 0;
}

// ... and gives the buffer back: for a launch that cannot keep prepared polygons at all (another kernel variant, a frame in
// bands, no room in the budgets).  A launch whose inputs merely differ from the last one's keeps the buffer - a camera that
// moves and stops would free and allocate 2 GB each time.  (hipFree waits for the device: no launch still loads from it.)
static void release_prepared_polygons(frame_pipeline* frames) {
	forget_prepared_polygons(frames);
	if (!frames || (!frames->prepared.buffer && !frames->prepared.terms)) return;
	(void) hipFree(frames->prepared.buffer);
	(void) hipFree(frames->prepared.terms);
	frames->prepared.buffer = NULL;
	frames->prepared.terms = NULL;
	frames->prepared.buffer_quads = frames->prepared.terms_quads = 0;
}

// Band step 4b: decides how this launch gets its prepared polygons -> f->prepared_mode, f->prepared
//   loading  when the cache holds the polygons of exactly these inputs and the launch that stored them has completed (the
//            event is queried, never waited for: until it completes, launches run plain) or runs on this launch's stream
//   storing  when the inputs are those of the launch before and nothing is stored or being stored
//   plain    otherwise - a moving frame pays a memcmp that fails early
static int choose_prepared_mode(application_t* app, frame_plan* f, frame_context* frame, hipStream_t stream) {
	const shade_params& p = f->p;
	f->prepared_mode = kPreparedPlain;
	f->prepared = NULL;
	f->terms = NULL;
	frame_pipeline* frames = f->frames;
	if (!frames) return 0;
	prepared_cache* cache = &frames->prepared;
	cache->last_mode = kPreparedPlain;
	if (!frame || f->prepared_quads == 0 || !prepared_polygons_possible(app, f)) {
		release_prepared_polygons(frames);
		++cache->launches[kPreparedPlain];
		return 0;
	}
	const shading_pass_t* pass = &app->shading_pass;
	prepared_arrangement arrangement;
	memset(&arrangement, 0, sizeof(arrangement));
	arrangement.first_block = p.first_block; arrangement.block_count = p.block_count; arrangement.thread_count = p.thread_count;
	arrangement.width = p.width; arrangement.height = p.height;
	arrangement.tile_size = p.tile_size; arrangement.rank = p.rank; arrangement.rank_count = p.rank_count;
	arrangement.tiles_x = p.tiles_x; arrangement.tile_count = p.tile_count; arrangement.slab_layout = p.slab_layout;
	arrangement.light_count = p.light_count; arrangement.max_light_vertex_count = p.max_light_vertex_count;
	arrangement.strategy = (uint32_t) f->strategy; arrangement.technique = (uint32_t) f->technique; arrangement.capacity = (uint32_t) f->capacity;
	arrangement.arithmetic_mode = (uint32_t) pass->arithmetic_mode;
	arrangement.inputs_generation = frames->inputs_generation;
	arrangement.build_serial = app->scene.acceleration_structure.build_serial;
	arrangement.ltc_serial = app->ltc_table.upload_serial;
	arrangement.ltc_resolution = p.ltc_resolution; arrangement.ltc_layer_count = p.ltc_layer_count;
	arrangement.visibility = p.visibility; arrangement.positions = p.positions; arrangement.normals_and_tex_coords = p.normals_and_tex_coords;
	arrangement.material_indices = p.material_indices; arrangement.material_constants = p.material_constants;
	arrangement.ltc_rgba = p.ltc_rgba; arrangement.ltc_rg = p.ltc_rg;
	const size_t size = sizeof(arrangement) + pass->constants_size;
	if (grow_bytes(&cache->scratch, &cache->scratch_capacity, size) || grow_bytes(&cache->seen, &cache->seen_capacity, size)) {
		printf("Failed to allocate %zu bytes for the inputs of the prepared polygons.\n", size);
		forget_prepared_polygons(frames);
		return 1;
	}
	uint8_t* now = cache->scratch;
	memcpy(now, &arrangement, sizeof(arrangement));
	memcpy(now + sizeof(arrangement), pass->constants_host, pass->constants_size);
	memset(now + sizeof(arrangement) + offsetof(per_frame_constants_t, noise_random_numbers), 0, sizeof(((per_frame_constants_t*) NULL)->noise_random_numbers));
	if (cache->seen_size != size || memcmp(now, cache->seen, size) != 0) {
		// other inputs: whatever is stored, or being stored, is of no use to anybody any more
		memcpy(cache->seen, now, size);
		cache->seen_size = size;
		cache->state = kCacheEmpty;
		++cache->launches[kPreparedPlain];
		return 0;
	}
	if (cache->state == kCachePending) {
		hipError_t stored = hipEventQuery(cache->stored);
		if (stored == hipSuccess) cache->state = kCacheValid;
		else {
			// (hipErrorNotReady is an answer, not an error: it must not meet the launch checks below)
			(void) hipGetLastError();
			// A launch on the stream of the storing launch runs behind it whatever the event says - the stream is in order -,
			// so it loads: frames that are submitted in a burst on ONE stream (frames_in_flight <= 1) load from the third on
			// instead of running plain until somebody waits.  Other streams are never made to wait for the storing launch.
			if (stream != cache->stored_stream) ++cache->waited;
		}
	}
	if (cache->state == kCacheValid || (cache->state == kCachePending && stream == cache->stored_stream)) {
		// (the terms were filled behind the storing launch, in front of the event: they are as complete as the polygons)
		const bool with_terms = cache->terms != NULL && cache->terms_quads != 0;
		f->prepared_mode = with_terms ? kPreparedLoadingTerms : kPreparedLoading;
		cache->last_mode = kPreparedLoading;
		f->prepared = cache->buffer;
		f->terms = with_terms ? cache->terms : NULL;
		++(with_terms ? cache->loaded_with_terms : cache->loaded_without_terms);
	}
	else if (cache->state == kCacheEmpty) {
		// (plan_bands() has found room for the buffer.  One of another size goes first: freeing waits for the device, so no launch
		// still loads from it, and the bytes that the statistics report are those of this arrangement.)
		if (cache->buffer && cache->buffer_quads != f->prepared_quads) {
			(void) hipFree(cache->buffer);
			cache->buffer = NULL;
			cache->buffer_quads = 0;
		}
		if (grow_device_buffer(&cache->buffer, &cache->buffer_quads, f->prepared_quads, sizeof(uint4), "Failed to allocate %.1f MiB for the prepared polygons.\n")) return 1;
		// the terms by the same rules; an arrangement without room for them keeps none
		if (cache->terms && cache->terms_quads != f->terms_quads) {
			(void) hipFree(cache->terms);
			cache->terms = NULL;
			cache->terms_quads = 0;
		}
		if (f->terms_quads != 0 && grow_device_buffer(&cache->terms, &cache->terms_quads, f->terms_quads, sizeof(float4), "Failed to allocate %.1f MiB for the sector terms.\n")) return 1;
		// launches in flight on other streams may still load what an earlier arrangement stored here.  (A launch outside the
		// pipeline runs behind finish_frames(), join_frame_pipeline(): it waits for events that it is behind already.)
		for (uint32_t c = 0; c != VKR_MAX_FRAMES_IN_FLIGHT; ++c) {
			frame_context* other = &frames->contexts[c];
			if (other != frame && other->recorded) (void) hipStreamWaitEvent(stream, other->done, 0);
		}
		f->prepared_mode = cache->last_mode = kPreparedStoring;
		f->prepared = cache->buffer;
	}
	// (mode 2 covers both loading kinds)
	++cache->launches[f->prepared_mode == kPreparedLoadingTerms ? kPreparedLoading : f->prepared_mode];
	return 0;
}

// ... and behind the launch: the terms kernel and the event of a storing launch, or nothing kept after a launch that failed
static void note_prepared_launch(const application_t* app, frame_plan* f, int status, hipStream_t stream) {
	frame_pipeline* frames = f->frames;
	if (!frames) return;
	if (status != 0) forget_prepared_polygons(frames);
	else if (f->prepared_mode == kPreparedStoring) {
		frames->prepared.stored_stream = stream;
		// the sector terms of what the launch has stored, on its stream: the event that lets other streams load lies behind both
		if (frames->prepared.terms) {
			const sector_terms_launch_function_t fill = g_sector_terms_launchers[app->shading_pass.arithmetic_mode];
			// (a kernel that the library lacks is an error, not a reason to load without terms)
			if (!fill || fill(f->capacity, frames->prepared.buffer, frames->prepared.terms, f->p.thread_count, f->p.light_count, stream) != 0) {
				printf("Failed to launch the kernel that fills the sector terms.\n");
				forget_prepared_polygons(frames);
				return;
			}
		}
		if (hipEventRecord(frames->prepared.stored, stream) == hipSuccess) frames->prepared.state = kCachePending;
		else forget_prepared_polygons(frames);
	}
}

// Band step 5: the shading kernel, or the error display's; < 0: no such kernel variant was built
static int launch_shading(const application_t* app, const frame_plan* f, hipStream_t stream) {
	const int mode = app->shading_pass.arithmetic_mode;
	const shade_params* p = &f->p;
	if (f->error_mode != kErrorNone)
		return g_error_launchers[mode](has_specular_technique(&app->render_settings), f->technique, f->capacity, f->error_mode, p, p->block_count, stream);
	if (f->prepared_mode != kPreparedPlain) {
		// (a variant that prepared_polygons_possible() promises and the library lacks is an error, not a reason to run plain)
		const prepared_launch_function_t launch = g_prepared_launchers[mode][f->strategy - kStrategySeparately];
		return launch ? launch(f->technique, f->capacity, f->prepared_mode, f->prepared, f->terms, p, p->block_count, stream) : -1;
	}
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

// Diagnostics: replays the rays that the last frame queued and counts the work of the
// traversal (profiles/ cites these numbers; not part of the frame).
__global__ void __launch_bounds__(256) k_traversal_statistics(bvh_view bvh, ray_stream stream, unsigned long long* out) {
	uint32_t queue = blockIdx.y;
	uint32_t size = stream.sizes[queue];
	unsigned long long visits = 0, tests = 0, blocked_rays = 0, rays = 0, wave_steps = 0;
	for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < ((size + 63u) & ~63u); i += gridDim.x * 256u) {
		uint32_t my_visits = 0;
		size_t slot = (size_t) queue * stream.capacity + i;
		if (i < size && stream.records[slot] != kNullRay) {
			float4 a = stream.origins[ray_record_thread(stream.thread_bits, stream.records[slot])], b = stream.directions[slot];
			f3 o = mk3(a.x, a.y, a.z), d = mk3(b.x, b.y, b.z);
			float t_max = b.w;
			grid_ray ray = make_grid_ray(bvh, o, d);
			uint32_t node = 0;
			bool blocked = false;
			++rays;
			while (t_max >= 1.0e-3f && node < bvh.node_count && !blocked) {
				uint4 n = bvh.nodes[node];
				bool is_leaf = (n.w & kLeafBit) != 0;
				bool hit = ray_box(n, ray, 1.0e-3f, t_max);
				++my_visits;
				if (hit && is_leaf) {
					const float4* t = bvh.triangles + 3 * (size_t) (n.w & ~kLeafBit);
					float dist;
					++tests;
					blocked = ray_triangle<false>(t[0], t[1], t[2], o, d, 1.0e-3f, t_max, dist);
				}
				node = (hit || is_leaf) ? node + 1 : n.w;
			}
			blocked_rays += blocked ? 1 : 0;
		}
		visits += my_visits;
		// steps the wave needs for these 64 rays = longest ray
		uint32_t longest = my_visits;
		for (int offset = 32; offset > 0; offset >>= 1) longest = max(longest, (uint32_t) __shfl_xor((int) longest, offset));
		if ((threadIdx.x & 63u) == 0) wave_steps += longest;
		atomicMax(out + 5, (unsigned long long) my_visits);
	}
	atomicAdd(out + 0, rays); atomicAdd(out + 1, visits); atomicAdd(out + 2, tests);
	atomicAdd(out + 3, blocked_rays); atomicAdd(out + 4, wave_steps);
}

// The same for the four-wide tree: "visits" are fetched nodes (dependent loads), out[5] the longest
// ray's, wave steps the longest ray of each group of 64; out[6] counts tested boxes, out[7] the
// deepest stack a ray reached, out[8] the rays whose stack outgrows the `lds_entries` entries that
// trace_shadow_rays_wide keeps in LDS (it holds the next item on the stack too: one entry more than the
// scheme here), out[9] the node visits of the rays that end up blocked
__global__ void __launch_bounds__(256) k_traversal_statistics_wide(bvh_view bvh, const uint4* wide_nodes, ray_stream stream, uint32_t lds_entries, unsigned long long* out) {
	uint32_t queue = blockIdx.y;
	uint32_t size = stream.sizes[queue];
	unsigned long long visits = 0, tests = 0, blocked_rays = 0, rays = 0, wave_steps = 0, boxes = 0, beyond_lds = 0, blocked_visits = 0;
	for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < ((size + 63u) & ~63u); i += gridDim.x * 256u) {
		uint32_t my_visits = 0;
		size_t slot = (size_t) queue * stream.capacity + i;
		if (i < size && stream.records[slot] != kNullRay) {
			float4 a = stream.origins[ray_record_thread(stream.thread_bits, stream.records[slot])], b = stream.directions[slot];
			f3 o = mk3(a.x, a.y, a.z), d = mk3(b.x, b.y, b.z);
			float t_max = b.w;
			wide_ray ray = make_wide_ray(make_grid_ray(bvh, o, d));
			uint32_t stack[kWideStackMax];
			uint32_t depth = 0, deepest = 0, item = 0;
			bool blocked = false, done = !(t_max >= 1.0e-3f);
			++rays;
			while (!done) {
				if (item & kLeafBit) {
					const float4* t = bvh.triangles + 3 * (size_t) (item & ~kLeafBit);
					float dist;
					++tests;
					blocked = ray_triangle<false>(t[0], t[1], t[2], o, d, 1.0e-3f, t_max, dist);
					if (blocked) break;
					item = 0xFFFFFFFFu;
				}
				else {
					const uint4* n = wide_nodes + 4 * (size_t) item;
					uint4 qx = n[0], qy = n[1], qz = n[2], link = n[3];
					const uint32_t x[4] = {qx.x, qx.y, qx.z, qx.w}, y[4] = {qy.x, qy.y, qy.z, qy.w}, z[4] = {qz.x, qz.y, qz.z, qz.w}, links[4] = {link.x, link.y, link.z, link.w};
					++my_visits;
					item = 0xFFFFFFFFu;
					// the order of trace_shadow_rays_wide: child 0 next, then 1, 2, 3 (pushed last to first)
					for (int c = 3; c >= 0; --c) {
						if (links[c] == kWideEmpty) continue;
						++boxes;
						if (!wide_ray_box(x[c], y[c], z[c], ray, 1.0e-3f, t_max)) continue;
						if (item != 0xFFFFFFFFu && depth < kWideStackMax) stack[depth++] = item;
						item = links[c];
					}
					deepest = max(deepest, depth);
				}
				if (item == 0xFFFFFFFFu) {
					if (depth == 0) done = true;
					else item = stack[--depth];
				}
			}
			blocked_rays += blocked ? 1 : 0;
			blocked_visits += blocked ? my_visits : 0u;
			beyond_lds += (deepest + 1u > lds_entries) ? 1 : 0;
			atomicMax(out + 7, (unsigned long long) deepest);
		}
		visits += my_visits;
		uint32_t longest = my_visits;
		for (int offset = 32; offset > 0; offset >>= 1) longest = max(longest, (uint32_t) __shfl_xor((int) longest, offset));
		if ((threadIdx.x & 63u) == 0) wave_steps += longest;
		atomicMax(out + 5, (unsigned long long) my_visits);
	}
	atomicAdd(out + 0, rays); atomicAdd(out + 1, visits); atomicAdd(out + 2, tests);
	atomicAdd(out + 3, blocked_rays); atomicAdd(out + 4, wave_steps); atomicAdd(out + 6, boxes);
	if (beyond_lds) atomicAdd(out + 8, beyond_lds);
	if (blocked_visits) atomicAdd(out + 9, blocked_visits);
}

// the wavefront buffers of the most recent launch with wavefront rays (the last band of the last frame), or NULL
static const wavefront_buffers* last_launch_buffers(const application_t* app) {
	const frame_pipeline* frames = (const frame_pipeline*) app->shading_pass.wavefront;
	return frames ? &frames->contexts[frames->last].buffers : NULL;
}

extern "C" int get_traversal_statistics(application_t* app, uint64_t out_statistics[6]) {
	const wavefront_buffers* w = last_launch_buffers(app);
	if (!w || !w->ray_directions || !app->shading_pass.use_ray_tracing || app->shading_pass.inline_rays) {
		printf("get_traversal_statistics() needs a frame rendered with wavefront shadow rays.\n");
		return 1;
	}
	uint64_t all[12];
	int failed = get_traversal_statistics_of_tree(app, app->scene.acceleration_structure.wide_nodes && !app->shading_pass.binary_traversal, all);
	memcpy(out_statistics, all, sizeof(uint64_t) * 6);
	return failed;
}

extern "C" int get_traversal_statistics_of_tree(application_t* app, VkBool32 wide_tree, uint64_t out_statistics[12]) {
	const frame_pipeline* frames = (const frame_pipeline*) app->shading_pass.wavefront;
	const wavefront_buffers* w = last_launch_buffers(app);
	const acceleration_structure_t* structure = &app->scene.acceleration_structure;
	if (!w || !w->ray_directions || !app->shading_pass.use_ray_tracing || app->shading_pass.inline_rays || (wide_tree && !structure->wide_nodes)) {
		printf("get_traversal_statistics_of_tree() needs a frame rendered with wavefront shadow rays (and the tree it is asked about).\n");
		return 1;
	}
	unsigned long long* counters = NULL;
	if (hip_failed(hipMalloc(&counters, sizeof(unsigned long long) * 12), "allocating traversal counters")) return 1;
	hipStream_t stream = (hipStream_t) app->device.stream;
	(void) finish_frames(app);
	(void) hipMemsetAsync(counters, 0, sizeof(unsigned long long) * 12, stream);
	bvh_view bvh = make_bvh_view(structure);
	// (the queues of the most recent launch - the last band of the last frame - with the sizes the resolve kernel kept)
	ray_stream rays = {w->ray_directions, w->ray_records, w->ray_origins, w->ray_queue_size + kRayCounterCount, w->queue_capacity, w->thread_bits, w->thread_count};
	if (wide_tree) k_traversal_statistics_wide<<<dim3(16, kRayQueueCount), 256, 0, stream>>>(bvh, (const uint4*) structure->wide_nodes, rays, frames->wide_stack_lds, counters);
	else k_traversal_statistics<<<dim3(16, kRayQueueCount), 256, 0, stream>>>(bvh, rays, counters);
	int failed = vkr_copy_to_host(out_statistics, counters, sizeof(uint64_t) * 12, &app->device);
	(void) hipFree(counters);
	return failed;
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

// {mode of the last launch, bytes of the buffer, launches plain / storing / loading, launches that found the storing one
// incomplete, state, budget in MiB} of the prepared polygon cache (include/vkr_shading_pass.h)
extern "C" int get_prepared_polygon_statistics(application_t* app, uint64_t out_statistics[8]) {
	memset(out_statistics, 0, 8 * sizeof(uint64_t));
	const frame_pipeline* frames = (const frame_pipeline*) app->shading_pass.wavefront;
	if (!frames) return 1;
	const prepared_cache* cache = &frames->prepared;
	out_statistics[0] = cache->last_mode;
	out_statistics[1] = (uint64_t) cache->buffer_quads * sizeof(uint4);
	for (int i = 0; i != 3; ++i) out_statistics[2 + i] = cache->launches[i];
	out_statistics[5] = cache->waited;
	out_statistics[6] = cache->state;
	out_statistics[7] = cache->budget_mib;
	return 0;
}

// {bytes of the buffer of the sector terms, loading launches with terms, loading launches without} (include/vkr_shading_pass.h)
extern "C" int get_sector_terms_statistics(application_t* app, uint64_t out_statistics[3]) {
	memset(out_statistics, 0, 3 * sizeof(uint64_t));
	const frame_pipeline* frames = (const frame_pipeline*) app->shading_pass.wavefront;
	if (!frames) return 1;
	const prepared_cache* cache = &frames->prepared;
	out_statistics[0] = (uint64_t) cache->terms_quads * sizeof(float4);
	out_statistics[1] = cache->loaded_with_terms;
	out_statistics[2] = cache->loaded_without_terms;
	return 0;
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
