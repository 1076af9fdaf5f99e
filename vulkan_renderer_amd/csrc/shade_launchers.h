// The host-side launchers of the kernel variant units, declared once: shading_variants.hip and
// shading_error_variants.hip define them and include this header, so that a definition whose parameters differ
// from what the callers (shading_pass.hip, device_probes.hip) see does not compile.
// All return 0 on success, 1 on a launch error and -1 if the combination was not built.
#pragma once
#include "shading_kernel.h"

// vkr_launch_shade_<mode>_<strategy>, mode: the arithmetic mode, with light textures compiled in as textured_<mode>
typedef int (*launch_function_t)(int technique, int capacity, int rays, const vkr::shade_params* p, unsigned int grid_x, void* stream);
#define VKR_DECLARE_LAUNCH(mode, s) extern "C" int vkr_launch_shade_##mode##_##s(int technique, int capacity, int rays, const vkr::shade_params* p, unsigned int grid_x, void* stream);
#define VKR_DECLARE_LAUNCHES(mode) VKR_DECLARE_LAUNCH(mode, 0) VKR_DECLARE_LAUNCH(mode, 1) VKR_DECLARE_LAUNCH(mode, 2) VKR_DECLARE_LAUNCH(mode, 3) VKR_DECLARE_LAUNCH(mode, 4)
VKR_DECLARE_LAUNCHES(libm) VKR_DECLARE_LAUNCHES(fast) VKR_DECLARE_LAUNCHES(exact)
VKR_DECLARE_LAUNCHES(textured_libm) VKR_DECLARE_LAUNCHES(textured_fast) VKR_DECLARE_LAUNCHES(textured_exact)

// the launchers that exist once per arithmetic mode (shading_error_variants.hip): a function type and <name>_libm, _fast, _exact
#define VKR_DECLARE_MODE_LAUNCHES(type, name, ...) typedef int (*type)(__VA_ARGS__); \
	extern "C" int name##_libm(__VA_ARGS__); extern "C" int name##_fast(__VA_ARGS__); extern "C" int name##_exact(__VA_ARGS__);
VKR_DECLARE_MODE_LAUNCHES(error_launch_function_t, vkr_launch_error_display, int combined_path, int technique, int capacity, int error_mode, const vkr::shade_params* p, unsigned int grid_x, void* stream)
VKR_DECLARE_MODE_LAUNCHES(resolve_launch_function_t, vkr_launch_resolve_materials, const vkr::shade_params* p, float* pixel_materials, void* stream)
VKR_DECLARE_MODE_LAUNCHES(sampler_launch_function_t, vkr_launch_texture_sampler, const vkr::shade_params* p, const uint32_t descriptor[4], const float* inputs, float* out_rgba, uint32_t count, void* stream)
// [arithmetic_mode_t]
#define VKR_MODE_LAUNCHERS(name) {name##_libm, name##_fast, name##_exact}
