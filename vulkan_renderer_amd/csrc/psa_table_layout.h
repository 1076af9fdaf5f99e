// The layout of what the projected solid angle samplers keep outside the registers - the polygon tables in LDS and the
// sector terms in device memory - as far as the host needs it to size buffers (shade_params.h).  The tables and terms
// themselves are polygon_sampling.h's (psa_compact, sector_terms).
#pragma once
#include <stdint.h>

namespace vkr {

constexpr int kPsaTableSlots(int V) { return 2 * V + 1; }
constexpr uint32_t kPsaTableStride = 64;  // threads of a shading workgroup (one wave, shade_params.h kShadeThreads)

// ---- sector terms kept in device memory (kept_polygons.h "Sector terms that are still true") ------------------------
// Per thread of the launch, light, polygon (diffuse, specular) and decentral sector k < V - 1 the eight sector_terms as
// two quads, [light][polygon][sector][half][thread]: half 0 = fin0 fin1 fin2 fout0, half 1 = fout1 fout2 in_rs out_rs.
typedef float sector_terms_quad __attribute__((ext_vector_type(4)));
constexpr int kSectorTermQuads(int v) { return 2 * 2 * (v - 1); }  // per thread and light
// the quad of (polygon, sector, half) in the column of a thread and light, in quads of a whole launch (thread_count each)
constexpr int sector_terms_quad_index(int v, int polygon, uint32_t sector, int half) { return (polygon * (v - 1) + (int) sector) * 2 + half; }

}  // namespace vkr
