// What the device file encoders (jpeg_encoder.hip, hdr_encoder.hip, png_encoder.hip) share: the slots that files leave the
// device through.  None of it knows a format.  The protocol:
//   - a slot's record in device memory is the size of the file in the first 8 of 16 bytes, then the file;
//   - a slot's staging memory has the layout of the record, is pinned and mapped into the device's address space: the
//     copy-out kernel writes it, the host reads it after the slot's event;
//   - an encode on a slot waits for the event of the slot's previous encode, whatever streams the two run on: the
//     scratch memory of the slot is free once that one is through;
//   - a slot can be ended once an encode with a copy-out has been enqueued on it in full (`begun`).
#ifndef VKR_OUTPUT_SLOTS_H
#define VKR_OUTPUT_SLOTS_H
#include "host/vkr_internal.h"
#include <hip/hip_runtime.h>

constexpr uint32_t kMaxOutputSlots = VKR_MAX_FRAMES_IN_FLIGHT + 1;

// Walks one allocation and hands out its pieces, each at a multiple of 256 bytes.  Without a base it only sizes, so that
// one listing of the fields serves both for the size to allocate and for the pointers.
struct output_carver {
	uint8_t* base;
	size_t total;
	template <typename T> void take(T*& field, size_t count) {
		size_t at = vkr_carve(&total, count * sizeof(T));
		field = base ? (T*) (base + at) : NULL;
	}
};

// Takes the format's own scratch buffers of slot `slot_index` into its named fields; `format_state` is what the format
// passed to create_output_slots()
typedef void (*output_slot_layout)(output_carver& carve, void* format_state, uint32_t slot_index);

struct output_slot {
	uint8_t* record;
	// temporary storage of the format's hipcub scans
	uint8_t* scan_storage;
	// the staging memory, and its address on the device
	uint8_t *staging, *staging_device;
	hipEvent_t done;
	bool begun;
};

struct output_slots {
	// "JPEG", "HDR", "PNG": for messages
	const char* format;
	void* stream;
	uint32_t slot_count;
	// the 16-byte units of a record: the size, then the file's capacity rounded up
	uint64_t record_units;
	size_t scan_bytes;
	void* scratch;
	// the one buffer that all slots read (tables, a header)
	uint8_t* shared;
	output_slot slots[kMaxOutputSlots];
};

bool valid_output_extent(uint32_t width, uint32_t height);

// The refusals of create_*_encoder(): no device, an extent outside 1 ... 65535, a slot count outside 1 ... kMaxOutputSlots
int check_output_arguments(const char* format, const device_t* device, uint32_t width, uint32_t height, uint32_t slot_count);

// Fills *slots, which is zeroed: one cleared device allocation for `shared_bytes` bytes copied from `shared`, and per
// slot what `layout` takes, a record for a file of `capacity` bytes with `spare_bytes` behind it and `scan_bytes` of
// scan storage; per slot the staging memory and the event.  After a failure destroy_output_slots() cleans up.
int create_output_slots(output_slots* slots, const char* format, const device_t* device, uint32_t slot_count, uint64_t capacity, size_t spare_bytes, size_t scan_bytes,
                        const void* shared, size_t shared_bytes, output_slot_layout layout, void* format_state);

// Waits for the encodes in flight and frees everything
void destroy_output_slots(output_slots* slots);

// 0 if `slots` exists and has this slot
int check_output_slot(const output_slots* slots, uint32_t slot_index);

// The head of an enqueue: *stream is the caller's stream or else the encoder's, and waits for the slot's previous encode
int begin_output_enqueue(output_slots* slots, uint32_t slot_index, void* stream_or_null, hipStream_t* stream);

// The tail of an enqueue: copies the record out with `copy_out_workgroups` workgroups (0: the file stays on the device),
// looks for launch errors, records the slot's event and, with a copy-out, notes that the slot can be ended
int finish_output_enqueue(output_slots* slots, uint32_t slot_index, hipStream_t stream, uint32_t copy_out_workgroups);

// end_*_encode(): refuses a slot that does not exist or never began, waits for the slot's encode and gives the file in
// the staging memory
int end_output_encode(output_slots* slots, uint32_t slot_index, const uint8_t** bytes, uint64_t* size);

#endif
