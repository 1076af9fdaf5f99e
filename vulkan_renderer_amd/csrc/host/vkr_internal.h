/* Internal helpers shared by the host-side C files of libvkr_shading.so. */
#ifndef VKR_INTERNAL_H
#define VKR_INTERNAL_H
#include "vkr_shading_pass.h"
#include "vkr_hip.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>

#define VKR_PI_F 3.1415926535897932384626433832795f
#define VKR_COUNT_OF(a) (sizeof(a) / sizeof((a)[0]))

#ifdef __cplusplus
extern "C" {
#endif

/*! malloc'ed copy of a string, NULL for NULL */
char* vkr_copy_string(const char* s);
/*! malloc'ed concatenation of count strings */
char* vkr_concatenate(uint32_t count, const char* const* pieces);

/*! Device memory helpers (device.c).  All return 0 on success and print the
	HIP error otherwise.  A NULL device makes uploads a no-op that yields NULL. */
int vkr_device_alloc(void** out, const device_t* device, size_t size, const char* what);
void vkr_device_free(void* pointer, const device_t* device);
int vkr_device_upload(void** out, const device_t* device, const void* host, size_t size, const char* what);
int vkr_host_alloc_pinned(void** out, size_t size);
/* output_encoding.hip: an empty kernel on `stream` (create_hip_device() warms the queues up with it) */
int vkr_launch_empty_kernel(void* stream);
/* fills the per-device tables of the kernels (sRGB code thresholds) and waits for it (output_encoding.hip) */
int vkr_fill_device_tables(void* stream);
/* ray_queries.hip: frees the stack buffer that the wide ray queries keep per HIP device (destroy_hip_device() calls it) */
void vkr_free_ray_query_buffers(int32_t hip_device);
void vkr_host_free_pinned(void* pointer);
int vkr_copy_to_device_async(void* device_pointer, const void* host, size_t size, const device_t* device);
int vkr_copy_to_host(void* host, const void* device_pointer, size_t size, const device_t* device);

/*! image_writers.c: what write_jpeg(), write_hdr_file() and write_png_file() are.  Writes the `size` bytes to a new file
	at `path`; 1, behind a message, if that fails */
int vkr_write_file(const char* path, const uint8_t* bytes, uint64_t size);

/*! ltc_table.c: what load_ltc_table() and fit_ltc_table() share.  Quantises fresnel_count * resolution^2 fits of five
	floats (the layout of the fit<i>.dat files) to host_rgba / host_rg, uploads them and sets the lookup constants.
	Overwrites *table; on failure prints the reason, leaves it zeroed and returns 1. */
int vkr_fill_ltc_table(ltc_table_t* table, const device_t* device, const float* fits, uint32_t resolution, uint32_t fresnel_count);

/*! textures.c: a material texture decoded to RGBA8, all mip levels one after the other */
typedef struct vkr_host_texture_s {
	uint32_t width, height, mip_count, srgb;
	uint8_t* texels;
	uint64_t texel_count;
} vkr_host_texture_t;
/*! 0 on success, 1 if the file is absent, 2 if it is invalid, 3 if its format is not decoded here */
int vkr_load_texture_rgba8(vkr_host_texture_t* out, const char* path);
void vkr_free_host_texture(vkr_host_texture_t* texture);
void vkr_decode_bc1_block(const uint8_t block[8], uint8_t out_rgba[64], int has_alpha);
void vkr_decode_bc5_block(const uint8_t block[16], uint8_t out_rgba[64]);
/*! scene.c: the sRGB -> linear table of the texture samplers (identical to oracle_srgb_table) */
void vkr_fill_srgb_table(float table[256]);

/*! texture_conversion.c: the highest level convert_texture() filters (extents up to 4096) */
#define VKR_TEXTURE_CONVERSION_MAX_LEVEL 12

/*! scene_export.c, for export_scene() of scene_export.hip (include/vkr_scene_export.h).  factor = scale / (hi - lo) and
	offset = -lo * factor per axis, both 0 where hi == lo; zeros of lo become +0 */
struct exported_scene_s;
struct scene_export_source_s;
void vkr_scene_export_box_constants(float factor[3], float offset[3], float lo[3], const float hi[3], float scale);
void vkr_scene_export_dequantization(struct exported_scene_s* scene, const float quantization_factor[3], const float lo[3], const float hi[3]);
/*! the substituted names and the material count; 1 when out of memory (free_exported_scene() cleans up) */
int vkr_scene_export_copy_names(struct exported_scene_s* scene, const struct scene_export_source_s* source);

/*! 4x4 inverse with the operation order of reference math_utilities.h:24-47 */
void vkr_matrix_inverse(float inverse[4][4], const float matrix[4][4]);
/*! reference math_utilities.h:50-57 */
uint32_t vkr_wang_random_number(uint32_t seed);

/*! Builds the BVH over the mesh with the given acceleration_structure_builder_t
	(include/vkr_scene.h) and derives both traversal layouts of csrc/lbvh.h from it */
int vkr_build_acceleration_structure(acceleration_structure_t* structure, const device_t* device, const mesh_t* mesh, int builder);
/*! sah_bvh.c: malloc'ed nodes (8 floats each, depth-first) and triangles (12 floats per leaf slot) */
int vkr_build_sah_bvh_host(const mesh_t* mesh, float pad, float** out_nodes, float** out_triangles, uint32_t* out_node_count);
void vkr_destroy_acceleration_structure(acceleration_structure_t* structure, const device_t* device);
/*! bvh_build.hip, shared with the refit of bvh_refit.hip: the next acceleration_structure_t.build_serial of the process
	(thread-safe), the padding of the boxes of a mesh, and grid_origin / grid_inverse_cell for a padded root box */
uint32_t vkr_next_build_serial(void);
float vkr_bvh_padding(const mesh_t* mesh);
void vkr_choose_bvh_grid(acceleration_structure_t* structure, const float lo[3], const float hi[3]);
/*! bvh_refit.hip: frees acceleration_structure_t.refit_state (vkr_destroy_acceleration_structure() calls it) */
void vkr_free_refit_state(acceleration_structure_t* structure, const device_t* device);

/*! slab_assembly.hip: scatters all-gathered slabs (format: slab_format_t of vkr_slab_exchange.h)
	into a frame on the given hipStream_t */
int vkr_assemble_slabs_on_stream(application_t* app, const void* gathered_slabs, void* out_frame, int format, void* stream);
/* (frame_transfers.hip) `event`, a hipEvent_t, marks the end of a reader of [target, target + bytes): the next frame that
   writes that range waits for it in front of the kernel that writes */
void vkr_note_target_reader(application_t* app, void* event, const void* target, size_t bytes);
void vkr_forget_target_reader(application_t* app, void* event);
/* (frame_transfers.hip) makes hipStream_t `stream` wait for the frames in flight, the most recent one of every frame stream
   (nothing to wait for without the frame pipeline: such frames ran on device->stream) */
int vkr_order_behind_frames_in_flight(application_t* app, void* stream);
/* (frame_transfers.hip) for a writer of [target, target + bytes) outside the pass: makes `stream` wait for the read-backs and
   noted readers of that range, as a frame that writes it does */
void vkr_order_target_write(application_t* app, const void* target, size_t bytes, void* stream);
/* (device.c) creates the frame streams 0 ... count - 1 of the device that do not exist yet */
int vkr_ensure_frame_streams(device_t* device, uint32_t count);

#ifdef __cplusplus
}
#endif

#endif
