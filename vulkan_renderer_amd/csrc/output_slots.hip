// The slots of the device file encoders (output_slots.h states the protocol):
//   k_copy_record_out   the size record and that many bytes into the slot's pinned staging memory
#include "output_slots.h"

namespace {

// Sixteen bytes per lane into host memory.
__global__ void __launch_bounds__(256) k_copy_record_out(const uint4* record, uint4* staging, uint64_t capacity_units) {
	uint64_t units = min(1 + (*(const uint64_t*) record + 15) / 16, capacity_units);
	for (uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x; i < units; i += (uint64_t) gridDim.x * 256) staging[i] = record[i];
}

void lay_out(output_slots* slots, output_carver& carve, size_t spare_bytes, size_t shared_bytes, output_slot_layout layout, void* format_state) {
	carve.take(slots->shared, shared_bytes);
	for (uint32_t i = 0; i != slots->slot_count; ++i) {
		output_slot& slot = slots->slots[i];
		layout(carve, format_state, i);
		carve.take(slot.record, slots->record_units * 16 + spare_bytes);
		carve.take(slot.scan_storage, slots->scan_bytes ? slots->scan_bytes : 1);
	}
}

}  // namespace

bool valid_output_extent(uint32_t width, uint32_t height) { return width != 0 && height != 0 && width <= 65535 && height <= 65535; }

int check_output_arguments(const char* format, const device_t* device, uint32_t width, uint32_t height, uint32_t slot_count) {
	if (!device) {
		printf("The %s encoder runs on the device: it has no host build.\n", format);
		return 1;
	}
	if (!valid_output_extent(width, height)) {
		printf("A file of the %s encoder is between 1 x 1 and 65535 x 65535 pixels, not %u x %u.\n", format, width, height);
		return 1;
	}
	if (slot_count == 0 || slot_count > kMaxOutputSlots) {
		printf("The %s encoder has 1 to %u slots, not %u.\n", format, kMaxOutputSlots, slot_count);
		return 1;
	}
	return 0;
}

int create_output_slots(output_slots* slots, const char* format, const device_t* device, uint32_t slot_count, uint64_t capacity, size_t spare_bytes, size_t scan_bytes,
                        const void* shared, size_t shared_bytes, output_slot_layout layout, void* format_state) {
	hipStream_t stream = (hipStream_t) device->stream;
	slots->format = format;
	slots->stream = device->stream;
	slots->slot_count = slot_count;
	slots->record_units = 1 + (capacity + 15) / 16;
	slots->scan_bytes = scan_bytes;
	output_carver carve = {NULL, 0};
	lay_out(slots, carve, spare_bytes, shared_bytes, layout, format_state);
	size_t total = carve.total;
	// k_copy_record_out copies whole 16-byte units, the rest of the size record and the tail behind the file included:
	// cleared once, no stale device memory reaches the host
	if (hip_failed(hipMalloc(&slots->scratch, total), "allocating the scratch memory of a file encoder")
		|| hip_failed(hipMemsetAsync(slots->scratch, 0, total, stream), "clearing the scratch memory of a file encoder")
		|| hip_failed(hipStreamSynchronize(stream), "clearing the scratch memory of a file encoder")) return 1;
	carve = {(uint8_t*) slots->scratch, 0};
	lay_out(slots, carve, spare_bytes, shared_bytes, layout, format_state);
	if (hip_failed(hipMemcpy(slots->shared, shared, shared_bytes, hipMemcpyHostToDevice), "uploading what the slots of a file encoder share")) return 1;
	for (uint32_t i = 0; i != slot_count; ++i) {
		output_slot& slot = slots->slots[i];
		if (hip_failed(hipHostMalloc((void**) &slot.staging, slots->record_units * 16, hipHostMallocDefault), "allocating the pinned staging memory of a file encoder")
			|| hip_failed(hipHostGetDevicePointer((void**) &slot.staging_device, slot.staging, 0), "mapping the staging memory of a file encoder")
			|| hip_failed(hipEventCreateWithFlags(&slot.done, hipEventDisableTiming), "creating the event of a slot")) return 1;
	}
	return 0;
}

void destroy_output_slots(output_slots* slots) {
	for (uint32_t i = 0; i != kMaxOutputSlots; ++i) {
		output_slot& slot = slots->slots[i];
		if (slot.done) {
			(void) hipEventSynchronize(slot.done);
			(void) hipEventDestroy(slot.done);
		}
		if (slot.staging) (void) hipHostFree(slot.staging);
	}
	if (slots->scratch) (void) hipFree(slots->scratch);
	memset(slots, 0, sizeof(*slots));
}

int check_output_slot(const output_slots* slots, uint32_t slot_index) {
	if (slots && slot_index < slots->slot_count) return 0;
	printf("Slot %u is not a slot of this %s encoder.\n", slot_index, slots ? slots->format : "file");
	return 1;
}

int begin_output_enqueue(output_slots* slots, uint32_t slot_index, void* stream_or_null, hipStream_t* stream) {
	*stream = (hipStream_t) (stream_or_null ? stream_or_null : slots->stream);
	return hip_failed(hipStreamWaitEvent(*stream, slots->slots[slot_index].done, 0), "ordering an encode behind the slot's previous one");
}

int finish_output_enqueue(output_slots* slots, uint32_t slot_index, hipStream_t stream, uint32_t copy_out_workgroups) {
	output_slot& slot = slots->slots[slot_index];
	if (copy_out_workgroups) k_copy_record_out<<<copy_out_workgroups, 256, 0, stream>>>((const uint4*) slot.record, (uint4*) slot.staging_device, slots->record_units);
	if (hip_failed(hipGetLastError(), "encoding a file") || hip_failed(hipEventRecord(slot.done, stream), "recording the end of an encode")) return 1;
	if (copy_out_workgroups) slot.begun = true;
	return 0;
}

int end_output_encode(output_slots* slots, uint32_t slot_index, const uint8_t** bytes, uint64_t* size) {
	if (check_output_slot(slots, slot_index)) return 1;
	output_slot& slot = slots->slots[slot_index];
	if (!slot.begun) {
		printf("The %s encode of slot %u is ended without having begun.\n", slots->format, slot_index);
		return 1;
	}
	if (hip_failed(hipEventSynchronize(slot.done), "waiting for an encode")) return 1;
	*size = *(const uint64_t*) slot.staging;
	*bytes = slot.staging + 16;
	return 0;
}
