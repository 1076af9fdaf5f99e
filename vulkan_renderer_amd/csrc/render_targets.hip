// The render targets, the primary visibility pass that fills the visibility buffer, and the blocking transfers
// of the targets (reading a frame back as the reference's implement_screenshot does, src/main.c:1719).
#include "pass_internal.h"
#include "lbvh.h"            // the visibility pass: closest_front_hit
#include "shading_inputs.h"  // ... and the constant loads

using namespace vkr;

// ---- render targets --------------------------------------------------------------

extern "C" void destroy_render_targets(render_targets_t* targets, const device_t* device) {
	vkr_device_free(targets->visibility_buffer, device);
	vkr_device_free(targets->radiance, device);
	vkr_device_free(targets->encoded, device);
	memset(targets, 0, sizeof(*targets));
}

extern "C" int create_render_targets(render_targets_t* targets, const device_t* device, const swapchain_t* swapchain) {
	memset(targets, 0, sizeof(*targets));
	if (!device) {
		printf("Render targets live in device memory; a HIP device is required.\n");
		return 1;
	}
	size_t pixels = (size_t) swapchain->extent.width * swapchain->extent.height;
	if (pixels == 0) return 2;  // reference main.c:1865: a minimised window is not an error
	targets->extent = swapchain->extent;
	// slabs are padded to whole tiles, so leave room for one extra row and column of 64-pixel tiles
	size_t padded = ((size_t) swapchain->extent.width + 64) * ((size_t) swapchain->extent.height + 64);
	if (vkr_device_alloc(&targets->visibility_buffer, device, sizeof(uint32_t) * pixels, "the visibility buffer")
		|| vkr_device_alloc(&targets->radiance, device, sizeof(float) * 4 * padded, "the radiance target")
		|| vkr_device_alloc(&targets->encoded, device, 4 * pixels, "the encoded output"))
	{
		destroy_render_targets(targets, device);
		return 1;
	}
	hipStream_t stream = (hipStream_t) device->stream;
	if (hip_failed(hipMemsetAsync(targets->visibility_buffer, 0xFF, sizeof(uint32_t) * pixels, stream), "clearing the visibility buffer")) {
		destroy_render_targets(targets, device);
		return 1;
	}
	return 0;
}

// ---- primary visibility ------------------------------------------------------------

__global__ void __launch_bounds__(256) k_primary_visibility(const uint8_t* constants, bvh_view bvh, uint32_t* visibility, uint32_t width, uint32_t height, float near, float far) {
	uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	uint32_t px = blockIdx.x * 16 + ((wave & 1) << 3) + (lane & 7);
	uint32_t py = blockIdx.y * 16 + ((wave >> 1) << 3) + (lane >> 3);
	if (px >= width || py >= height) return;
	float fx = (float) px, fy = (float) py;
	f3 ray = mk3(
		(load_f(constants, 96) * fx + load_f(constants, 100) * fy) + load_f(constants, 104),
		(load_f(constants, 112) * fx + load_f(constants, 116) * fy) + load_f(constants, 120),
		(load_f(constants, 128) * fx + load_f(constants, 132) * fy) + load_f(constants, 136));
	f3 origin = load_f3(constants, 144);
	// The unnormalised ray direction has view-space depth 1 (it is the unprojection of
	// clip-space w = 1), so the depth range [near, far] is the parameter range.
	visibility[(size_t) py * width + px] = closest_front_hit(bvh, origin, ray, near, far);
}

extern "C" int render_visibility_pass(application_t* app) {
	// frames in flight read the visibility buffer that this pass overwrites
	if (finish_frames(app)) return 1;
	mark_inputs_changed(app);
	shading_pass_t* pass = &app->shading_pass;
	const acceleration_structure_t* as = &app->scene.acceleration_structure;
	if (!as->triangle_vertices || !pass->constants_device) {
		printf("The visibility pass needs an acceleration structure and a shading pass.\n");
		return 1;
	}
	if (upload_constants(app, (hipStream_t) app->device.stream)) return 1;
	bvh_view bvh = make_bvh_view(as);
	uint32_t width = app->swapchain.extent.width, height = app->swapchain.extent.height;
	dim3 grid((width + 15) / 16, (height + 15) / 16);
	k_primary_visibility<<<grid, 256, 0, (hipStream_t) app->device.stream>>>((const uint8_t*) pass->constants_device, bvh, (uint32_t*) app->render_targets.visibility_buffer,
		width, height, app->scene_specification.camera.near, app->scene_specification.camera.far);
	return hip_failed(hipGetLastError(), "rendering the visibility pass");
}

// ---- transfers -------------------------------------------------------------------

// a target of the frame's extent, pixel_bytes per pixel, behind the frames in flight
static int read_back_target(application_t* app, void* host, const void* target, size_t pixel_bytes) {
	if (finish_frames(app)) return 1;
	size_t pixels = (size_t) app->swapchain.extent.width * app->swapchain.extent.height;
	return vkr_copy_to_host(host, target, pixel_bytes * pixels, &app->device);
}
extern "C" int read_back_radiance(application_t* app, float* host_rgba) { return read_back_target(app, host_rgba, app->render_targets.radiance, sizeof(float) * 4); }
extern "C" int read_back_encoded(application_t* app, uint8_t* host_rgba8) { return read_back_target(app, host_rgba8, app->render_targets.encoded, 4); }
extern "C" int read_back_visibility(application_t* app, uint32_t* host_primitives) { return read_back_target(app, host_primitives, app->render_targets.visibility_buffer, sizeof(uint32_t)); }
extern "C" int upload_visibility(application_t* app, const uint32_t* host_primitives) {
	// a blocking copy outside the streams: nothing may still be reading the old buffer
	if (wait_for_device(&app->device)) return 1;
	mark_inputs_changed(app);
	size_t pixels = (size_t) app->swapchain.extent.width * app->swapchain.extent.height;
	if (hip_failed(hipMemcpy(app->render_targets.visibility_buffer, host_primitives, sizeof(uint32_t) * pixels, hipMemcpyHostToDevice), "uploading the visibility buffer")) return 1;
	return 0;
}
