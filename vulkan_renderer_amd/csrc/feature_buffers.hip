// Feature buffers (include/vkr_feature_buffers.h), host side: the argument checks, the parameters of the launch from the
// application and the choice of the arithmetic mode's launcher (feature_buffers_variants.hip).  No kernel and no state.
#include "pass_internal.h"
#include "shade_launchers.h"
#include "vkr_feature_buffers.h"

using namespace vkr;

// [arithmetic_mode_t]
static const feature_launch_function_t g_feature_launchers[3] = VKR_MODE_LAUNCHERS(vkr_launch_feature_buffers);

extern "C" int render_feature_buffers(application_t* app, const feature_buffers_t* buffers) {
	const shading_pass_t* pass = app ? &app->shading_pass : NULL;
	if (!pass || !buffers || pass->variant < 0 || !pass->constants_device || !pass->constants_ring
		|| pass->arithmetic_mode < 0 || pass->arithmetic_mode >= arithmetic_mode_count)
	{
		printf("render_feature_buffers() needs a shading pass created by create_shading_pass().\n");
		return 1;
	}
	shade_params p;
	memset(&p, 0, sizeof(p));
	p.positions = (const uint2*) app->scene.mesh.positions;
	p.normals_and_tex_coords = (const uint2*) app->scene.mesh.normals_and_tex_coords;
	p.material_indices = (const uint8_t*) app->scene.mesh.material_indices;
	p.material_constants = (const float*) app->scene.materials.constants;
	p.visibility = (const uint32_t*) app->render_targets.visibility_buffer;
	p.width = app->swapchain.extent.width;
	p.height = app->swapchain.extent.height;
	if (!p.positions || !p.normals_and_tex_coords || !p.material_indices || !p.material_constants || !p.visibility || p.width == 0 || p.height == 0
		|| p.width != app->render_targets.extent.width || p.height != app->render_targets.extent.height)
	{
		printf("render_feature_buffers() needs a loaded scene and render targets of the swapchain extent on the device.\n");
		return 1;
	}
	if (app->tile_schedule.rank_count > 1 || app->tile_schedule.slab_layout) {
		printf("render_feature_buffers() writes whole frames of one rank: no slab layout, no more than one rank.\n");
		return 1;
	}
	bool wanted = false, aligned = true;
	for (int i = 0; i != pixel_feature_count; ++i) {
		wanted = wanted || buffers->images[i] != NULL;
		aligned = aligned && ((uintptr_t) buffers->images[i] & 15u) == 0;
	}
	if (!wanted || !aligned) {
		printf("render_feature_buffers() needs at least one image, and every image 16-byte aligned.\n");
		return 1;
	}
	// textured scene: the material textures are sampled in the kernel (pass->pixel_materials is left alone)
	const int textured = app->scene.materials.textured && app->scene.materials.texture_descriptors;
	if (textured) {
		p.texture_descriptors = (const uint32_t*) app->scene.materials.texture_descriptors;
		p.texels = (const uint32_t*) app->scene.materials.texels;
		p.srgb_table = (const float*) app->scene.materials.srgb_table;
	}
	hipStream_t stream = (hipStream_t) app->device.stream;
	if (upload_constants(app, stream)) return 1;
	p.constants = (const uint8_t*) pass->constants_device;
	if (g_feature_launchers[pass->arithmetic_mode](&p, buffers->images, &buffers->reprojection_matrix[0][0], textured, stream)) {
		printf("Failed to launch the feature buffer kernel.\n");
		return 1;
	}
	return 0;
}

extern "C" int encode_feature_preview(application_t* app, uint32_t feature, const void* image, void* out_rgba8, float range_low, float range_high) {
	if (!app || !image || !out_rgba8 || ((uintptr_t) image & 15u) != 0 || ((uintptr_t) out_rgba8 & 3u) != 0
		|| app->swapchain.extent.width == 0 || app->swapchain.extent.height == 0)
	{
		printf("encode_feature_preview() needs a feature image (16-byte aligned), an output (4-byte aligned) and an extent.\n");
		return 1;
	}
	if (feature >= (uint32_t) pixel_feature_count) {
		printf("encode_feature_preview(): %u is no pixel_feature_t.\n", feature);
		return 1;
	}
	const bool uses_range = feature == (uint32_t) pixel_feature_position || feature == (uint32_t) pixel_feature_reprojection;
	// (written so that a NaN fails)
	if (uses_range && !(range_high > range_low)) {
		printf("encode_feature_preview() needs range_low < range_high for this feature.\n");
		return 1;
	}
	launch_feature_preview(feature, image, out_rgba8, app->swapchain.extent.width, app->swapchain.extent.height, range_low, range_high, (hipStream_t) app->device.stream);
	return hip_failed(hipGetLastError(), "encoding the feature preview");
}
