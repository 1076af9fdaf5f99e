// What a frame moves between host and device, and who has to wait for whom around it: the ring of constant buffers
// (write_constants src/main.c:2114), the read-back slots, and the readers of a frame's target outside the pass.  No kernel.
#include "frame_pipeline.h"

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

void destroy_constants_ring(shading_pass_t* pass, const device_t* device) {
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

int create_constants_ring(shading_pass_t* pass, const device_t* device) {
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

// ... and before the caller destroys such an event
extern "C" void vkr_forget_target_reader(application_t* app, void* event) {
	read_back_state* rb = (read_back_state*) app->shading_pass.readback;
	if (!rb || !event) return;
	for (uint32_t i = 0; i != kReadBackSlots; ++i)
		if (rb->reader_event[i] == (hipEvent_t) event) rb->reader_event[i] = NULL;
	if (app->shading_pass.wait_before_next_frame == event) app->shading_pass.wait_before_next_frame = NULL;
}

void destroy_read_back(shading_pass_t* pass) {
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

void wait_for_read_backs_of(shading_pass_t* pass, const void* target, size_t bytes, hipStream_t stream) {
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
