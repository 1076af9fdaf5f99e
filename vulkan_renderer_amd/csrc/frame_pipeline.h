// What the units of the frame pipeline share and nobody else includes (shading_pass.hip, frame_transfers.hip,
// light_shaft_step.hip, prepared_polygons.hip, pass_diagnostics.hip, traversal_statistics.hip): the pipeline's structs and the functions that one of
// these units calls in another.  The narrow header of the rest of the pass is pass_internal.h.
#pragma once
#include "pass_internal.h"
#include "kept_inputs.h"

// events of a timed frame: its start, the start and the end of the (last band's) shading kernel, its end
constexpr uint32_t kTimingFrameStart = 0, kTimingShadingStart = 1, kTimingShadingEnd = 2, kTimingFrameEnd = 3, kTimingEvents = 4;

inline hipEvent_t timing_event(const shading_pass_t* pass, uint32_t slot, uint32_t which) { return ((hipEvent_t*) pass->timing_ring)[kTimingEvents * slot + which]; }

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
	// most recent launch with these buffers (light_shaft_step.hip shaft_arrangement).  The shaft kernel keeps a verdict only
	// while these bytes are the next launch's, too.
	kept_inputs shaft_seen;
	size_t shaft_words;
	// ... and per light the plane-space rectangle that the shading kernel tests its rays against
	float4* shaft_rectangles;
	size_t shaft_rectangle_count;
	// ... and per pair kShaftListMax triangle slots: the occluder lists (VKR_SHAFT_LISTS)
	float* shaft_lists;
	size_t shaft_list_words;
	// the second polygon table of every shading workgroup, for the kernel variants that keep one table in LDS only
	// (shade_params.h psa_table_in_memory); allocated when such a variant first runs
	float2* psa_table_memory;
	size_t psa_table_bytes;
};

// The prepared polygons of the most recent launches (kept_polygons.h "Prepared polygons that are still true")
enum { kCacheEmpty = 0, kCachePending = 1, kCacheValid = 2 };
struct prepared_cache {
	uint4* buffer;  // the second argument of the storing and the loading kernel, allocated when a launch first stores
	size_t buffer_quads;
	// the sector terms of the polygons in `buffer` (kept_polygons.h "Sector terms that are still true"): the third argument of
	// the kernel that loads with terms, allocated, retained and released by the rules of `buffer`, and filled behind the storing
	// launch, in front of `stored`.  terms_quads: its size, 0: the launches of this arrangement load without terms
	float4* terms;
	size_t terms_quads;
	// a byte image of everything the preparation reads (prepared_polygons.hip prepared_arrangement), of the most recent
	// launch that the cache could serve
	kept_inputs seen;
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
	// part of what the kept results are derived from (launch_inputs below)
	uint32_t inputs_generation;
	// where a band step puts the inputs of a launch together before it compares them with the kept copy: run_light_shafts()
	// with the context's, then choose_prepared_mode() with the cache's - one after the other, never both at once
	inputs_scratch scratch;
	// the polygon tables in device memory (wavefront_buffers::psa_table_memory) of the frames without wavefront rays, which
	// own no context
	wavefront_buffers device_stream_buffers;
	// the prepared polygons that the shading kernel keeps while its inputs stand still (prepared_polygons.hip): one
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
	// (read, with VKR_SHAFT_LISTS, VKR_SHAFT_REST and VKR_SHAFT_MAX_STEPS, by create_light_shafts())
	// VKR_WIDE_REFILL, VKR_WIDE_REFILL_BELOW (round 5): ensure_frames()
	uint32_t wide_stack_lds, wide_refill, wide_refill_below, wavefront_budget_mib, band_count, light_shafts, shaft_lists, shaft_rest, shaft_max_steps;
};

// What render_pass() decides about a frame before its first band (plan_frame, plan_bands); the band steps read it
struct frame_plan {
	vkr::shade_params p;     // the parameters of every launch of the frame; a band step adds the band's blocks and buffers
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
	// (table_in_memory: the kernel variants that keep one of their two polygon tables in device memory, shade_params.h psa_table_in_memory)
	bool table_in_memory, hidden_terms, base_color, use_wide_tree, textured, pipelined;
	uint32_t grid_blocks, table_bytes_per_workgroup, max_terms;
	// frames in flight (1: not pipelined), the bands of the frame, workgroups of the tracing kernels (wavefront rays only)
	uint32_t depth, band_count, blocks_per_band, trace_blocks;
	// bytes of the output this call writes (a slab in slab layout, else the frame): what pending read-backs are checked against
	size_t frame_output_bytes;
};

inline uint32_t environment_knob(const char* name, uint32_t fallback, uint32_t low, uint32_t high) {
	const char* text = getenv(name);
	if (!text || !text[0]) return fallback;
	long value = strtol(text, NULL, 10);
	return (uint32_t) (value < (long) low ? (long) low : (value > (long) high ? (long) high : value));
}

// grow_bytes() for a device buffer of `count` elements, whose content is not kept: a buffer that is too small is freed
// (while other frames may be in flight: hipFree waits for the device) and allocated anew.  On failure pointer and count
// are zero and `message` is printed, a format for the MiB that were asked for.
template <typename T>
inline int grow_device_buffer(T** buffer, size_t* count, size_t wanted, size_t element_bytes, const char* message) {
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

// the wavefront buffers of the most recent launch with wavefront rays (the last band of the last frame), or NULL
inline const wavefront_buffers* last_launch_buffers(const application_t* app) {
	const frame_pipeline* frames = (const frame_pipeline*) app->shading_pass.wavefront;
	return frames ? &frames->contexts[frames->last].buffers : NULL;
}

// The head of the byte image of either kept result (kept_inputs.h; shaft_arrangement, prepared_arrangement): the tiling
// of the launch, its lights, and what names the content behind the two pointers.  Who changes an input and how that shows
// here: a BVH build (scene load; mesh and materials are uploaded with it) gives the tree a new build_serial; whoever
// rewrites the visibility buffer or another input in device memory - render_visibility_pass, upload_visibility, a caller
// on its own through mark_inputs_changed() (INTEGRATION.md obliges it to) - bumps inputs_generation.
struct launch_inputs {
	uint32_t first_block, block_count, width, height, tile_size, rank, rank_count, tiles_x, tile_count, slab_layout;
	uint32_t light_count, max_light_vertex_count, inputs_generation, build_serial;
	const void *visibility, *positions;
};
static_assert(sizeof(launch_inputs) == 14 * 4 + 2 * sizeof(void*), "no padding: the struct is compared as bytes");

// (into an arrangement that has been cleared as a whole)
inline void fill_launch_inputs(launch_inputs& head, const vkr::shade_params& p, const frame_pipeline* frames, const acceleration_structure_t* structure) {
	head.first_block = p.first_block; head.block_count = p.block_count;
	head.width = p.width; head.height = p.height;
	head.tile_size = p.tile_size; head.rank = p.rank; head.rank_count = p.rank_count;
	head.tiles_x = p.tiles_x; head.tile_count = p.tile_count; head.slab_layout = p.slab_layout;
	head.light_count = p.light_count; head.max_light_vertex_count = p.max_light_vertex_count;
	head.inputs_generation = frames->inputs_generation;
	head.build_serial = structure->build_serial;
	head.visibility = p.visibility; head.positions = p.positions;
}

// ---- frame_transfers.hip ----
int create_constants_ring(shading_pass_t* pass, const device_t* device);
void destroy_constants_ring(shading_pass_t* pass, const device_t* device);
void destroy_read_back(shading_pass_t* pass);
// Makes `stream` wait for every pending copy that reads from [target, target + bytes): called in front of the kernel
// of a frame that writes its output (the resolve kernel with wavefront rays, the shading kernel otherwise)
void wait_for_read_backs_of(shading_pass_t* pass, const void* target, size_t bytes, hipStream_t stream);

// ---- light_shaft_step.hip ----
// the shaft knobs of a new pipeline; the shaft tables and the kept inputs of a set of buffers
void create_light_shafts(frame_pipeline* frames);
void destroy_light_shafts(wavefront_buffers* w);
// Band step 4: the shaft kernel of the band where the light shafts apply, its tables in p
int run_light_shafts(application_t* app, frame_plan* f, frame_context* frame, hipStream_t stream);

// ---- prepared_polygons.hip ----
// the cache's event and knobs of a new pipeline (non-zero: no event); everything the cache owns
int create_prepared_polygons(frame_pipeline* frames);
void destroy_prepared_polygons(frame_pipeline* frames);
// plan_bands(): f->prepared_quads and f->terms_quads, what fits beside `wavefront` bytes of wavefront buffers into `budget`
void plan_prepared_polygons(const application_t* app, frame_plan* f, double wavefront, double budget);
// Band step 4b: decides how this launch gets its prepared polygons -> f->prepared_mode, f->prepared, f->terms
int choose_prepared_mode(application_t* app, frame_plan* f, frame_context* frame, hipStream_t stream);
// band step 5 for every other mode than plain; < 0: no such kernel variant was built
int launch_prepared_shading(const application_t* app, const frame_plan* f, hipStream_t stream);
// ... and behind the launch: the terms kernel and the event of a storing launch, or nothing kept after a launch that failed
void note_prepared_launch(const application_t* app, frame_plan* f, int status, hipStream_t stream);
