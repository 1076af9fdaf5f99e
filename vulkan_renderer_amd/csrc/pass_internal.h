// What the units of the shading pass's host side share (the frame pipeline - shading_pass.hip and the units beside it -,
// render_targets.hip, output_encoding.hip, slab_assembly.hip, device_probes.hip): the functions that one unit calls in
// another.  Functions only: the pipeline's structs stay private to its own units (frame_pipeline.h).
// The library is built with -fvisibility=hidden, so none of these is exported.
#pragma once
#include "shade_params.h"
#include "host/vkr_internal.h"

// ---- the frame pipeline: frame_transfers.hip, shading_pass.hip (slab_tiling) ----
// Call behind a kernel on device->stream that reads a buffer frames in flight write (the radiance
// target, a caller's slab): the next frames wait for it before they resolve.
void note_target_reader(application_t* app);
// write_constants and, if the bytes changed, upload them into the next free slot on
// `stream`; in any case `stream` is made to wait for the upload of the slot it will read
int upload_constants(application_t* app, hipStream_t stream);
// The tiling of `rank`'s slab (p: width, height and tile schedule); returns the slab's pixel count.  Rank 0 owns the most
// tiles: its count is the stride of the slabs in a gathered buffer.
uint64_t slab_tiling(const application_t* app, uint32_t rank, vkr::shade_params& p);

// ---- output_encoding.hip ----
// queues the kernel that encodes pixel_count pixels (a multiple of four) as packed RGB8
void launch_encode_rgb8(const void* radiance, void* packed, uint64_t pixel_count, uint32_t frame_bits, int output_linear_rgb, hipStream_t stream);
// queues the kernel that turns a feature image (a pixel_feature_t of include/vkr_feature_buffers.h) into RGBA8: it lives
// beside the sRGB code that two of the previews are
void launch_feature_preview(uint32_t feature, const void* image, void* out_rgba8, uint32_t width, uint32_t height, float range_low, float range_high, hipStream_t stream);
