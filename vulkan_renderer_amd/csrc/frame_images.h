// What the units that work on whole frame images outside the pass share (frame_filter.hip, frame_history.hip and the
// resolve of frame_statistics.hip).  None of it knows what a unit computes.  The protocol:
//   - an object owns float4 images of one extent and one event; its public struct keeps them, a frame_image_set points
//     into that struct;
//   - a call checks its images in one order: the required ones and the alignment of all, then that the object was
//     created, then that no output overlaps an input, the other output or an image that the object owns;
//   - a call runs on device->stream.  begin_frame_call() puts it behind the frames in flight, which do not follow that
//     stream (an input may be a target of any of them), and behind the read-backs and noted readers of what it writes;
//   - finish_frame_call() records the object's event and, where a pass exists, notes it as a reader of every image of the
//     call: a later frame that writes one of them waits for it.  Only a pass writes frames, and it is the pass that
//     keeps the readers;
//   - destroying an object waits for device->stream (its kernels may still run), takes the event back from the pass,
//     destroys it and frees the images.
#ifndef VKR_FRAME_IMAGES_H
#define VKR_FRAME_IMAGES_H
#include "host/vkr_internal.h"
#include "device_math.h"
#include <hip/hip_runtime.h>

// ---- device side ---------------------------------------------------------------------------------------------------

namespace vkr {

VKR_DEV f3 rgb(float4 a) { return mk3(a.x, a.y, a.z); }
VKR_DEV f3 divide3_full_range(f3 a, f3 b) { return mk3(divide_full_range(a.x, b.x), divide_full_range(a.y, b.y), divide_full_range(a.z, b.z)); }
VKR_DEV f3 divide3_full_range(f3 a, float b) { return mk3(divide_full_range(a.x, b), divide_full_range(a.y, b), divide_full_range(a.z, b)); }
VKR_DEV f3 gmax3(float a, f3 b) { return mk3(gmax(a, b.x), gmax(a, b.y), gmax(a, b.z)); }

// m of the headers from a pixel of the modulation image
VKR_DEV f3 modulation_of(float4 a) { return mk3(gmax(a.x, 1.0f / 256.0f), gmax(a.y, 1.0f / 256.0f), gmax(a.z, 1.0f / 256.0f)); }

// The lane's pixel in a workgroup of 256 lanes: 16x16 pixels per workgroup, 8x8 per wave (the mapping of
// k_feature_buffers), so that what a wave reads or writes of an image at one offset - its own pixels, or one tap of a
// filter - is eight runs of 128 consecutive bytes
VKR_DEV void lane_pixel(uint32_t& lx, uint32_t& ly) {
	uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	lx = ((wave & 1) << 3) + (lane & 7);
	ly = ((wave >> 1) << 3) + (lane >> 3);
}

}  // namespace vkr

// ---- host side -----------------------------------------------------------------------------------------------------

constexpr uint32_t kMaxFrameImages = 8, kFrameCallInputs = 6, kFrameCallOutputs = 2;

// The images and the event that an object owns, as pointers into its public struct
struct frame_image_set {
	// "filter", "history": for messages
	const char* noun;
	uint32_t *width, *height;
	void** event;
	uint32_t count;
	void** images[kMaxFrameImages];
};

// The images of one call, NULL where the caller gives none
struct frame_call {
	// the function's name, for messages
	const char* function;
	const void* inputs[kFrameCallInputs];
	void* outputs[kFrameCallOutputs];
};

// Fills what `set` points to, which is zeroed: `set.count` images of the extent (0, 0: the swapchain's; at most
// `max_extent` either way), cleared if the caller may read one before a call wrote it, and the event.  `images_noun`:
// what the images are to the object, for the message.  After a failure everything is released again.
int create_frame_images(const frame_image_set& set, application_t* app, uint32_t width, uint32_t height, uint32_t max_extent, bool cleared, const char* images_noun);

// Waits for the calls in flight, frees everything and zeroes what `set` points to
void destroy_frame_images(const frame_image_set& set, application_t* app);

bool frame_images_created(const frame_image_set& set);

inline size_t frame_image_bytes(const frame_image_set& set) { return sizeof(float4) * (size_t) *set.width * *set.height; }

// 0 if `required` (whether the call has the images that it cannot do without) and every image is 16-byte aligned
int check_frame_call_images(const frame_call& call, bool required);

// 0 if no output overlaps an input, the other output or, with `own`, an image of that set
int check_frame_call_overlap(const frame_call& call, size_t bytes, const frame_image_set* own);

// The head of a call, behind its checks: orders device->stream, which is *stream, as the protocol says
int begin_frame_call(const frame_call& call, application_t* app, size_t bytes, hipStream_t* stream);

// The tail of a call, behind its launches: records `event` on device->stream (`what`: "marking ...", for a HIP error) and
// notes it as the reader of the call's images
int finish_frame_call(const frame_call& call, application_t* app, size_t bytes, void* event, const char* what);

#endif
