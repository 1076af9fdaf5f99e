/* Ray queries against the acceleration structure of a loaded scene: the caller's rays, closest hit and any hit.
   No reference counterpart: the reference traces rays only inside its shaders (VK_KHR_ray_query,
   src/shaders/shading_pass.frag.glsl:120-138). */
#ifndef VKR_RAY_QUERIES_H
#define VKR_RAY_QUERIES_H
#include "vkr_scene.h"

/*! A ray o + t d, t in [t_min, t_max].  The direction need not be normalised: t counts lengths of d. */
typedef struct ray_s {
	float origin[3], t_min, direction[3], t_max;
} ray_t;

/*! primitive: the index of the triangle in the scene file, 0xFFFFFFFF for a miss; t along the ray, u and v the
	barycentric coordinates of the second and third vertex */
typedef struct ray_hit_s {
	uint32_t primitive;
	float t, u, v;
} ray_hit_t;

/*! Which layout of the tree the rays walk (csrc/lbvh.h).  The answers do not depend on it. */
typedef enum ray_walk_e {
	/*! the four-wide tree if the scene has one whose stack the kernels provide, else the threaded binary tree: the wide
		walk was the faster one on every scene and ray set that was measured */
	ray_walk_auto = 0,
	ray_walk_binary,
	ray_walk_wide
} ray_walk_t;

typedef struct ray_query_options_s {
	/*! a ray_walk_t */
	uint32_t walk;
	/*! Stack entries per ray that the wide walk keeps in LDS, at most kWideStackLds (16, csrc/lbvh.h); deeper entries go
		to a buffer in device memory that the call sizes from acceleration_structure_t.wide_stack_need.  0: the default, 16.
		Tests shrink it to drive rays through that buffer. */
	uint32_t lds_stack_entries;
} ray_query_options_t;

/* ---- the calls -----------------------------------------------------------------------------------------------------

   rays, out_hits and out_blocked are device pointers to `count` records, rays and out_hits aligned to 16 bytes.  The
   kernels (csrc/ray_queries.hip) are enqueued on `stream`, a hipStream_t, or on device->stream if it is NULL, and the
   calls return once they are enqueued: ordering the buffers against other work is the caller's business.  The tree changes only in update_scene_geometry()
   (vkr_scene_update.h), which waits for the device first.  options NULL:
   the defaults (ray_walk_auto, 0).  The stack entries beyond LDS of the wide walk live in one buffer per HIP device (at
   most 256 MiB; more rays run in pieces) that the first call which needs it allocates and destroy_hip_device() frees;
   calls on different streams are ordered behind each other on the device for its sake.

   Both return 0 on success; count == 0 returns 0 and launches nothing.  They return 1 after printing one line, and write
   nothing, for: a scene without acceleration structure, device == NULL (there is no host build), count > 2^31, a
   walk that is no ray_walk_t, ray_walk_wide for a scene without wide_nodes or whose wide_stack_need exceeds
   kWideStackMax (128), and lds_stack_entries > kWideStackLds.

   The rules that follow are the interface; the numpy restatement vulkan_renderer_amd/ray_queries.py is held to them and
   gives the same bits.  All arithmetic is binary32, every operation rounded on its own (nothing contracted), divisions
   correctly rounded.  dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z; cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z,
   a.x b.y - a.y b.x).  The vertices p0, p1, p2 of a triangle are the de-quantised positions of the scene file,
   (float) q * dequantization_factor + dequantization_summand per coordinate.

   1. A triangle PASSES for a ray (o, d, t_min, t_max) if ray_triangle_edges<CULL_BACK>() of csrc/lbvh.h accepts it with the
      ray's own t_min and t_max - the operation order of oracle/oracle_bvh.c:128-144 and :190-206:
        e1 = p1 - p0, e2 = p2 - p0, p = cross(d, e2), det = dot(e1, p);
        two-sided: det != 0, with back-face culling: det > 0, else it fails;
        sign = det < 0 ? -1 : 1, adet = det * sign, s = o - p0;
        U = dot(s, p) * sign, and U >= 0 and U <= adet;
        q = cross(s, e1), V = dot(d, q) * sign, and V >= 0 and U + V <= adet;
        T = dot(e2, q) * sign, and T >= t_min * adet and T <= t_max * adet.
      Every comparison is written so that a NaN fails it.
   2. The values of a passing triangle are t = T / adet, u = U / adet, v = V / adet.
   3. trace_closest_hits() returns, of the passing triangles, the one with the smallest (t, primitive) in lexicographic
      order (a NaN t, which only rays with infinite components produce, counts as larger than every number), primitive
      being the index in the file.  The answer does not depend on the tree, on the walk or on how many leaves the builder
      has split a triangle into - for triangles that the ray meets at a cosine of incidence above 2^-10 (see below).
   4. A miss is {0xFFFFFFFF, +infinity, 0, 0}.
   5. trace_any_hits() writes 1 if any triangle passes the two-sided test, else 0.
   6. A ray with !(t_max >= t_min), with d = 0 or with a NaN among its eight floats misses (no triangle can pass).

   The tree only culls: boxes are tested against [t_min, min(t_max, best t so far)], widened by 2^-10 of either end on
   top of the outward rounding of the quantised boxes, because the t of rule 2 carries a relative error that grows with
   the obliquity of the triangle: a few 2^-24 over the cosine of the angle of incidence.  That is the bound
   of the promise of rule 3: the widening covers cosines down to about 2^-10 (0.06 degrees off the triangle's plane).  For a
   triangle that a ray grazes more flatly, the rounded t of another triangle, less than 2^-10 of t in front of it, may cull
   its box; nothing measures or proves what happens there, and the answer is then the rule's for the triangles that were
   not culled.  A triangle whose box survives is tested with the ray's own t_max, not
   the shrunk one: otherwise ties would depend on the order of the visits.  (closest_front_hit() of csrc/lbvh.h, which
   render_visibility_pass() uses, shrinks t_max like the oracle's loop does.)  A ray whose origin lies more than 2^16 cells of the
   tree's grid (two widths of the scene box) from the grid's origin, whose largest direction component is outside
   [2^-60, 2^60], or which has an infinite component there, is tested against every triangle: the slab arithmetic of the
   boxes is not exact enough for it, and the answer must not depend on that. */
VKR_API int trace_closest_hits(const scene_t* scene, const device_t* device, const ray_t* rays, uint64_t count,
                               VkBool32 cull_back_faces, ray_hit_t* out_hits, const ray_query_options_t* options, void* stream);
VKR_API int trace_any_hits(const scene_t* scene, const device_t* device, const ray_t* rays, uint64_t count,
                           uint8_t* out_blocked, const ray_query_options_t* options, void* stream);

#endif
