// The images, the event and the ordering of the units that work on whole frame images (frame_images.h states the protocol).
// Host code only: the device helpers of the header are instantiated by the kernels of their users.
#include "frame_images.h"

void destroy_frame_images(const frame_image_set& set, application_t* app) {
	// (the kernels of the last call may still read and write the images)
	if (*set.event && app && app->device.stream) (void) hipStreamSynchronize((hipStream_t) app->device.stream);
	if (*set.event) {
		// (the pass may still hold the event as the reader of a target)
		if (app) vkr_forget_target_reader(app, *set.event);
		(void) hipEventDestroy((hipEvent_t) *set.event);
		*set.event = NULL;
	}
	for (uint32_t i = 0; i != set.count; ++i) {
		if (*set.images[i]) (void) hipFree(*set.images[i]);
		*set.images[i] = NULL;
	}
	*set.width = *set.height = 0;
}

int create_frame_images(const frame_image_set& set, application_t* app, uint32_t width, uint32_t height, uint32_t max_extent, bool cleared, const char* images_noun) {
	if (!width && !height) {
		width = app->swapchain.extent.width;
		height = app->swapchain.extent.height;
	}
	if (!width || !height || width > max_extent || height > max_extent) {
		printf("A frame %s needs a width and a height between 1 and %u (an extent, or a swapchain extent).\n", set.noun, max_extent);
		return 1;
	}
	*set.width = width;
	*set.height = height;
	size_t bytes = frame_image_bytes(set);
	for (uint32_t i = 0; i != set.count; ++i) {
		void** image = set.images[i];
		bool allocated = hipMalloc(image, bytes) == hipSuccess;
		if (!allocated) *image = NULL;
		if (!allocated || (cleared && hipMemset(*image, 0, bytes) != hipSuccess)) {
			printf("Failed to allocate %.1f MiB for the %s of a %ux%u frame %s.\n", (double) set.count * bytes / 1048576.0, images_noun, width, height, set.noun);
			destroy_frame_images(set, app);
			return 1;
		}
	}
	char what[64];
	snprintf(what, sizeof(what), "creating the %s's event", set.noun);
	if (hip_failed(hipEventCreateWithFlags((hipEvent_t*) set.event, kSyncEventFlags), what)) {
		*set.event = NULL;
		destroy_frame_images(set, app);
		return 1;
	}
	return 0;
}

bool frame_images_created(const frame_image_set& set) {
	bool created = *set.event && *set.width && *set.height;
	for (uint32_t i = 0; i != set.count; ++i) created = created && *set.images[i];
	return created;
}

int check_frame_call_images(const frame_call& call, bool required) {
	bool aligned = true;
	for (const void* image : call.inputs) aligned = aligned && ((uintptr_t) image & 15u) == 0;
	for (const void* image : call.outputs) aligned = aligned && ((uintptr_t) image & 15u) == 0;
	if (required && aligned) return 0;
	printf("%s() needs colour, position, normal and out_colour, and every image 16-byte aligned.\n", call.function);
	return 1;
}

static bool overlap(const void* a, const void* b, size_t bytes) {
	const uint8_t* x = (const uint8_t*) a;
	const uint8_t* y = (const uint8_t*) b;
	return x && y && x < y + bytes && y < x + bytes;
}

int check_frame_call_overlap(const frame_call& call, size_t bytes, const frame_image_set* own) {
	bool overlapping = overlap(call.outputs[0], call.outputs[1], bytes);
	for (const void* output : call.outputs) {
		for (const void* input : call.inputs) overlapping = overlapping || overlap(output, input, bytes);
		for (uint32_t i = 0; own && i != own->count; ++i) overlapping = overlapping || overlap(output, *own->images[i], bytes);
	}
	if (!overlapping) return 0;
	if (own) printf("%s(): an output overlaps an input, the other output or an image of the %s.\n", call.function, own->noun);
	else printf("%s(): an output overlaps an input or the other output.\n", call.function);
	return 1;
}

int begin_frame_call(const frame_call& call, application_t* app, size_t bytes, hipStream_t* stream) {
	*stream = (hipStream_t) app->device.stream;
	if (vkr_order_behind_frames_in_flight(app, *stream)) return 1;
	for (void* output : call.outputs)
		if (output) vkr_order_target_write(app, output, bytes, *stream);
	return 0;
}

int finish_frame_call(const frame_call& call, application_t* app, size_t bytes, void* event, const char* what) {
	if (hip_failed(hipEventRecord((hipEvent_t) event, (hipStream_t) app->device.stream), what)) return 1;
	if (app->shading_pass.constants_device) {
		for (const void* input : call.inputs)
			if (input) vkr_note_target_reader(app, event, input, bytes);
		for (void* output : call.outputs)
			if (output) vkr_note_target_reader(app, event, output, bytes);
	}
	return 0;
}
