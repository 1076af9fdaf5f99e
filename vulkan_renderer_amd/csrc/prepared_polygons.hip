// The prepared polygon cache (kept_polygons.h "Prepared polygons that are still true", "Sector terms that are still
// true"): which launches keep prepared polygons, the room for them in the budgets, the state machine that
// decides whether a launch stores, loads or runs plain, and the launch of those kernel variants.  No kernel of its own.
#include "shade_launchers.h"
#include "frame_pipeline.h"

using namespace vkr;

// [arithmetic_mode_t][strategy - kStrategySeparately]: the kernels with kept prepared polygons; none in the fast mode
#define VKR_PREPARED_ROW(mode) {vkr_launch_shade_prepared_##mode##_2, vkr_launch_shade_prepared_##mode##_3, vkr_launch_shade_prepared_##mode##_4}
static const prepared_launch_function_t g_prepared_launchers[3][3] = {VKR_PREPARED_ROW(libm), {NULL, NULL, NULL}, VKR_PREPARED_ROW(exact)};
static const sector_terms_launch_function_t g_sector_terms_launchers[3] = {vkr_launch_sector_terms_libm, NULL, vkr_launch_sector_terms_exact};

int create_prepared_polygons(frame_pipeline* frames) {
	// VKR_PREPARED_POLYGONS_MIB: most device memory that the kept prepared polygons of a launch may take; 0: nothing is kept,
	// every launch prepares its polygons itself.  (Config 3 at 1920x1080 keeps 2 040 MiB: 2.09 M threads x 4 lights x 256 B.)
	// (with the sector terms of those polygons - as much again at V = 5 - where both fit: 4 080 MiB)
	frames->prepared.budget_mib = environment_knob("VKR_PREPARED_POLYGONS_MIB", 4096u, 0u, 262144u);
	// VKR_SECTOR_TERMS=0: the loading launches compute the terms of their sectors themselves
	frames->prepared.terms_enabled = environment_knob("VKR_SECTOR_TERMS", 1u, 0u, 1u);
	return hipEventCreateWithFlags(&frames->prepared.stored, kSyncEventFlags) != hipSuccess;
}

void destroy_prepared_polygons(frame_pipeline* frames) {
	(void) hipFree(frames->prepared.buffer);
	(void) hipFree(frames->prepared.terms);
	if (frames->prepared.stored) (void) hipEventDestroy(frames->prepared.stored);
	free_inputs(&frames->prepared.seen);
}

// Which launches can keep prepared polygons at all: the kernel variants of prepared_polygons_apply() (shade_params.h),
// untextured.  plan_prepared_polygons() adds: one launch per frame, and room in the budgets.
static bool prepared_polygons_possible(const application_t* app, const frame_plan* f) {
	return f->ray_mode == kRaysDeferredBlocks && f->error_mode == kErrorNone && !f->table_in_memory && !f->textured
		&& !f->p.light_texture_descriptors && app->shading_pass.arithmetic_mode != arithmetic_mode_fast && f->p.light_count != 0
		&& (f->technique == kTechniquePsa || f->technique == kTechniquePsaBiased) && f->strategy >= kStrategySeparately && f->strategy <= kStrategyRandom
		&& f->capacity >= 4 && f->capacity <= 5;
}

// The prepared polygons of a frame that is one launch (a frame in bands meets a context's buffers with another band each
// time, and config 4, the frame that is rendered in bands, has no such kernel variant): one buffer per pass, counted against
// the budget of the wavefront buffers like the shafts' tables, and against VKR_PREPARED_POLYGONS_MIB.  (bind_textures() runs
// after this: a frame with light textures is turned away by choose_prepared_mode().)
void plan_prepared_polygons(const application_t* app, frame_plan* f, double wavefront, double budget) {
	const prepared_cache* cache = &f->frames->prepared;
	f->prepared_quads = f->terms_quads = 0;
	if (f->band_count != 1 || cache->budget_mib == 0u || !prepared_polygons_possible(app, f)) return;
	const double own_budget = (double) cache->budget_mib * 1048576.0;
	const uint32_t thread_count = f->blocks_per_band * 256u;
	const size_t pairs = (size_t) thread_count * f->p.light_count;
	const size_t quads = pairs * (prepared_bytes_per_pair(f->capacity) / 16u);
	const double bytes = 16.0 * (double) quads;
	if (quads == 0 || bytes > own_budget || wavefront + bytes > budget) return;
	f->prepared_quads = quads;
	// the terms count against both budgets together with the polygons; where only the polygons fit, the launch loads without
	const size_t terms_quads = pairs * (sector_terms_bytes_per_pair(f->capacity) / 16u);
	const double both = bytes + 16.0 * (double) terms_quads;
	if (cache->terms_enabled && both <= own_budget && wavefront + both <= budget) f->terms_quads = terms_quads;
}

// Everything the preparation of a launch reads, as bytes: this struct and behind it the constants of the launch - camera,
// de-quantisation, roughness factor, the LTC table's lookup constants and every light's record - with the four noise
// words blanked, which only the samples read.  (The constants hold more than the preparation reads - exposure, the MIS
// visibility estimate: a change of those costs one plain and one storing launch and nothing else.)
// What lies behind the pointers is named by the serials of launch_inputs (frame_pipeline.h) and the LTC table's
// upload_serial.
struct prepared_arrangement {
	launch_inputs head;
	uint32_t thread_count, strategy, technique, capacity, arithmetic_mode, ltc_serial, ltc_resolution, ltc_layer_count;
	const void *normals_and_tex_coords, *material_indices, *material_constants, *ltc_rgba, *ltc_rg;
};
static_assert(sizeof(prepared_arrangement) == sizeof(launch_inputs) + 8 * 4 + 5 * sizeof(void*), "no padding: the struct is compared as bytes");

static void forget_prepared_polygons(frame_pipeline* frames) {
	if (!frames) return;
	frames->prepared.state = kCacheEmpty;
	forget_inputs(&frames->prepared.seen);
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

// A buffer of the cache for `wanted` quads (0: none).  One of another size goes first: freeing waits for the device, so no
// launch still loads from it, and the bytes that the statistics report are those of this arrangement.
template <typename T>
static int fit_cache_buffer(T** buffer, size_t* quads, size_t wanted, const char* message) {
	if (*buffer && *quads != wanted) {
		(void) hipFree(*buffer);
		*buffer = NULL;
		*quads = 0;
	}
	return grow_device_buffer(buffer, quads, wanted, sizeof(T), message);
}

//   loading  when the cache holds the polygons of exactly these inputs and the launch that stored them has completed (the
//            event is queried, never waited for: until it completes, launches run plain) or runs on this launch's stream
//   storing  when the inputs are those of the launch before and nothing is stored or being stored
//   plain    otherwise - a moving frame pays a memcmp that fails early
int choose_prepared_mode(application_t* app, frame_plan* f, frame_context* frame, hipStream_t stream) {
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
	fill_launch_inputs(arrangement.head, p, frames, &app->scene.acceleration_structure);
	arrangement.thread_count = p.thread_count;
	arrangement.strategy = (uint32_t) f->strategy; arrangement.technique = (uint32_t) f->technique; arrangement.capacity = (uint32_t) f->capacity;
	arrangement.arithmetic_mode = (uint32_t) pass->arithmetic_mode;
	arrangement.ltc_serial = app->ltc_table.upload_serial;
	arrangement.ltc_resolution = p.ltc_resolution; arrangement.ltc_layer_count = p.ltc_layer_count;
	arrangement.normals_and_tex_coords = p.normals_and_tex_coords;
	arrangement.material_indices = p.material_indices; arrangement.material_constants = p.material_constants;
	arrangement.ltc_rgba = p.ltc_rgba; arrangement.ltc_rg = p.ltc_rg;
	const size_t size = sizeof(arrangement) + pass->constants_size;
	uint8_t* now = begin_inputs(&cache->seen, &frames->scratch, size);
	if (!now) {
		printf("Failed to allocate %zu bytes for the inputs of the prepared polygons.\n", size);
		forget_prepared_polygons(frames);
		return 1;
	}
	memcpy(now, &arrangement, sizeof(arrangement));
	memcpy(now + sizeof(arrangement), pass->constants_host, pass->constants_size);
	memset(now + sizeof(arrangement) + offsetof(per_frame_constants_t, noise_random_numbers), 0, sizeof(((per_frame_constants_t*) NULL)->noise_random_numbers));
	if (!same_inputs(&cache->seen, now, size, 0, size)) {
		// other inputs: whatever is stored, or being stored, is of no use to anybody any more
		keep_inputs(&cache->seen, now, size);
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
		// (plan_bands() has found room for the buffers; an arrangement without room for the terms keeps none)
		if (fit_cache_buffer(&cache->buffer, &cache->buffer_quads, f->prepared_quads, "Failed to allocate %.1f MiB for the prepared polygons.\n")
			|| fit_cache_buffer(&cache->terms, &cache->terms_quads, f->terms_quads, "Failed to allocate %.1f MiB for the sector terms.\n"))
			return 1;
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

int launch_prepared_shading(const application_t* app, const frame_plan* f, hipStream_t stream) {
	// (a variant that prepared_polygons_possible() promises and the library lacks is an error, not a reason to run plain)
	const prepared_launch_function_t launch = g_prepared_launchers[app->shading_pass.arithmetic_mode][f->strategy - kStrategySeparately];
	return launch ? launch(f->technique, f->capacity, f->prepared_mode, f->prepared, f->terms, &f->p, f->p.block_count, stream) : -1;
}

void note_prepared_launch(const application_t* app, frame_plan* f, int status, hipStream_t stream) {
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
