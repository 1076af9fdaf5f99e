// Motion buffers (include/vkr_motion_buffers.h), host side: the argument checks, the parameters of the launch from the
// application and the choice of the arithmetic mode's launcher (motion_buffers_variants.hip).  No kernel and no state.
#include "pass_internal.h"
#include "shade_launchers.h"
#include "vkr_motion_buffers.h"

using namespace vkr;

// [arithmetic_mode_t]
static const motion_launch_function_t g_motion_launchers[3] = VKR_MODE_LAUNCHERS(vkr_launch_motion_buffers);

extern "C" int render_motion_buffers(application_t* app, const motion_buffers_t* buffers) {
	const shading_pass_t* pass = app ? &app->shading_pass : NULL;
	if (!pass || !buffers || pass->variant < 0 || !pass->constants_device || !pass->constants_ring
		|| pass->arithmetic_mode < 0 || pass->arithmetic_mode >= arithmetic_mode_count)
	{
		printf("render_motion_buffers() needs a shading pass created by create_shading_pass().\n");
		return 1;
	}
	shade_params p;
	memset(&p, 0, sizeof(p));
	p.positions = (const uint2*) app->scene.mesh.positions;
	// (named by intersect_primitive(), whose normals and texture coordinates this kernel never loads)
	p.normals_and_tex_coords = (const uint2*) app->scene.mesh.normals_and_tex_coords;
	p.visibility = (const uint32_t*) app->render_targets.visibility_buffer;
	p.width = app->swapchain.extent.width;
	p.height = app->swapchain.extent.height;
	if (!p.positions || !p.normals_and_tex_coords || !p.visibility || p.width == 0 || p.height == 0
		|| p.width != app->render_targets.extent.width || p.height != app->render_targets.extent.height)
	{
		printf("render_motion_buffers() needs a loaded scene and render targets of the swapchain extent on the device.\n");
		return 1;
	}
	if (app->tile_schedule.rank_count > 1 || app->tile_schedule.slab_layout) {
		printf("render_motion_buffers() writes whole frames of one rank: no slab layout, no more than one rank.\n");
		return 1;
	}
	void* const images[3] = {buffers->reprojection, buffers->previous_position, buffers->motion};
	bool wanted = false, aligned = ((uintptr_t) buffers->previous_positions & 7u) == 0;
	for (void* image : images) {
		wanted = wanted || image != NULL;
		aligned = aligned && ((uintptr_t) image & 15u) == 0;
	}
	if (!wanted || !aligned) {
		printf("render_motion_buffers() needs at least one image, every image 16-byte aligned and previous_positions 8-byte aligned.\n");
		return 1;
	}
	hipStream_t stream = (hipStream_t) app->device.stream;
	if (upload_constants(app, stream)) return 1;
	p.constants = (const uint8_t*) pass->constants_device;
	// (nothing moved: the mesh's own positions are the previous ones)
	const void* previous_positions = buffers->previous_positions ? buffers->previous_positions : (const void*) p.positions;
	if (g_motion_launchers[pass->arithmetic_mode](&p, previous_positions, images, &buffers->previous_matrix[0][0], stream)) {
		printf("Failed to launch the motion buffer kernel.\n");
		return 1;
	}
	return 0;
}
