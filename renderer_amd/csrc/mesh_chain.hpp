// mesh_chain.hpp — the per-mesh LOD chain of the batched-draws extension (mip_batch_draws_lods): filled by mip_set_mesh_table
// (api_context.hip) beside MeshEntry and MeshDraw, read by batch_lods_kernel.hpp only.
#pragma once

#include <cstdint>

namespace mip {

// One 64-byte line per mesh, gathered as 16-byte pieces: {n_lods, lod_base, len 0, len 1} {len 2..5} {offset 0..3}
// {offset 4, 5, -, -}. Levels at or above n_lods hold zeros.
struct alignas(64) MeshChain {
  uint32_t n_lods;
  uint32_t lod_base;         // sum of n_lods over the meshes in front of this one: the mesh's first bucket
  uint32_t index_len[6];     // MIP_MAX_LODS
  uint32_t index_offset[6];
  uint32_t pad[2];
};
static_assert(sizeof(MeshChain) == 64, "one line per mesh");

}  // namespace mip
