// Slabs -> frame: scatters the all-gathered slabs of the ranks (tile_schedule_t, host/slab_exchange.c) into a
// row-major frame, as float4, RGBA8 or packed RGB8.
#include "pass_internal.h"

using namespace vkr;

template <typename PIXEL>
__global__ void __launch_bounds__(256) k_assemble_frame(const PIXEL* slabs, PIXEL* frame, uint32_t width, uint32_t height, uint32_t tile_size, uint32_t tiles_x, uint32_t rank_count, uint64_t slab_stride) {
	uint32_t px = blockIdx.x * 16 + (threadIdx.x & 15), py = blockIdx.y * 16 + (threadIdx.x >> 4);
	if (px >= width || py >= height) return;
	uint32_t tx = px / tile_size, ty = py / tile_size;
	uint32_t tile = ty * tiles_x + tx;
	uint32_t rank = tile % rank_count, local_tile = tile / rank_count;
	uint32_t ix = px - tx * tile_size, iy = py - ty * tile_size;
	frame[(size_t) py * width + px] = slabs[rank * slab_stride + (size_t) local_tile * tile_size * tile_size + (size_t) iy * tile_size + ix];
}

extern "C" uint64_t get_slab_pixel_count(const application_t* app, uint32_t rank) {
	shade_params p;
	return slab_tiling(app, rank, p);
}

template <typename PIXEL>
static int assemble_slabs(application_t* app, const void* gathered_slabs, void* out_frame, hipStream_t stream) {
	shade_params p;
	uint64_t slab_stride = slab_tiling(app, 0, p);
	dim3 grid((p.width + 15) / 16, (p.height + 15) / 16);
	k_assemble_frame<PIXEL><<<grid, 256, 0, stream>>>((const PIXEL*) gathered_slabs, (PIXEL*) out_frame,
		p.width, p.height, p.tile_size, p.tiles_x, p.rank_count, slab_stride);
	return hip_failed(hipGetLastError(), "assembling the frame");
}

extern "C" int assemble_frame_from_slabs(application_t* app, const void* gathered_slabs, void* out_radiance) {
	// (the radiance target may still be written by frames in flight)
	if (finish_frames(app)) return 1;
	return assemble_slabs<float4>(app, gathered_slabs, out_radiance ? out_radiance : app->render_targets.radiance, (hipStream_t) app->device.stream);
}

extern "C" int assemble_encoded_frame_from_slabs(application_t* app, const void* gathered_slabs, void* out_encoded) {
	if (finish_frames(app)) return 1;
	return assemble_slabs<uint32_t>(app, gathered_slabs, out_encoded ? out_encoded : app->render_targets.encoded, (hipStream_t) app->device.stream);
}

// slabs of packed RGB8 (encode_slab_rgb8) -> RGBA8 frame; alpha of the encoded output is always
// 255.  A thread moves four pixels of one tile row: twelve bytes = three aligned dwords in
// (tile sizes are multiples of four), four pixels out.
__global__ void __launch_bounds__(256) k_assemble_frame_rgb8(const uint32_t* slabs, uint32_t* frame, uint32_t width, uint32_t height, uint32_t tile_size, uint32_t tiles_x, uint32_t rank_count, uint64_t slab_stride) {
	uint32_t px = 4u * (blockIdx.x * 64u + (threadIdx.x & 63u)), py = blockIdx.y * 4u + (threadIdx.x >> 6);
	if (px >= width || py >= height) return;
	uint32_t tx = px / tile_size, ty = py / tile_size;
	uint32_t tile = ty * tiles_x + tx;
	uint32_t rank = tile % rank_count, local_tile = tile / rank_count;
	uint32_t ix = px - tx * tile_size, iy = py - ty * tile_size;
	size_t pixel = rank * slab_stride + (size_t) local_tile * tile_size * tile_size + (size_t) iy * tile_size + ix;
	const uint32_t* source = slabs + 3 * (pixel / 4);
	uint32_t d0 = source[0], d1 = source[1], d2 = source[2];
	uint32_t out[4] = {d0 | 0xFF000000u, (d0 >> 24) | (d1 << 8) | 0xFF000000u, (d1 >> 16) | (d2 << 16) | 0xFF000000u, (d2 >> 8) | 0xFF000000u};
	uint32_t* target = frame + (size_t) py * width + px;
	for (uint32_t i = 0; i != 4 && px + i < width; ++i) target[i] = out[i];
}

static int assemble_rgb8_slabs(application_t* app, const void* gathered_slabs, void* out_encoded, hipStream_t stream) {
	shade_params p;
	uint64_t slab_stride = slab_tiling(app, 0, p);
	if (p.tile_size % 4 != 0) {
		printf("assemble_rgb8_frame_from_slabs() needs a tile size that is a multiple of four.\n");
		return 1;
	}
	dim3 grid((p.width + 255) / 256, (p.height + 3) / 4);
	k_assemble_frame_rgb8<<<grid, 256, 0, stream>>>((const uint32_t*) gathered_slabs, (uint32_t*) (out_encoded ? out_encoded : app->render_targets.encoded),
		p.width, p.height, p.tile_size, p.tiles_x, p.rank_count, slab_stride);
	return hip_failed(hipGetLastError(), "assembling the frame");
}

extern "C" int assemble_rgb8_frame_from_slabs(application_t* app, const void* gathered_slabs, void* out_encoded) {
	if (finish_frames(app)) return 1;
	return assemble_rgb8_slabs(app, gathered_slabs, out_encoded, (hipStream_t) app->device.stream);
}

// For host/slab_exchange.c: the scatter of gathered slabs on a stream of the caller's choice
// (the exchange stream, so that it does not wait for later frames), format as slab_format_t
extern "C" int vkr_assemble_slabs_on_stream(application_t* app, const void* gathered_slabs, void* out_frame, int format, void* stream) {
	if (format == 0) return assemble_slabs<float4>(app, gathered_slabs, out_frame ? out_frame : app->render_targets.radiance, (hipStream_t) stream);
	return assemble_rgb8_slabs(app, gathered_slabs, out_frame, (hipStream_t) stream);
}
