// cluster_triangle_plan.hpp — the arithmetic of mip_cull_cluster_triangles (extension, not reference behaviour) that is not a
// kernel: the index-overflow decision, the grids of the four kernels behind the cluster cull and the scratch they take, all
// pure functions of the call's bound on W. Plain C++, no HIP: api_cluster.hip and cluster_triangle_kernel.hpp call it,
// tests/native/cluster_triangle_plan_check.cpp enumerates it on the CPU over its decision edges.
#pragma once

#include "cluster_plan.hpp"

namespace mip {

constexpr uint32_t kClusterTriangleTileWords = kClusterItemTile / 64u;  // survive words of a tile of the test / write kernels
constexpr uint32_t kClusterTriangleStats = 6;                           // heads, surviving clusters, W, members, surviving triangles, triangles tested
static_assert(kClusterTriangleTileWords <= 64u, "the write kernel holds a tile's word totals one per lane");

// Whether a call whose items keep `triangles` triangles writes its stream (else MIP_ERR_CAPACITY, no command and no index
// written): the stream's 3 x triangles indices are within index_capacity and below 2^32 — firstIndex is a 32-bit word.
MIP_CLUSTER_HD constexpr bool cluster_triangle_index_fits(unsigned long long triangles, uint32_t index_capacity) {
  return triangles <= 0xFFFFFFFFull / 3ull && 3ull * triangles <= index_capacity;
}

// What the call launches and allocates behind mip_cull_clusters' count / scan / members / cull / heads. The test and the write
// kernel walk the cull kernel's item tiles, the commands kernel the head tiles; both grids are capped and loop as theirs do.
struct ClusterTrianglePlan {
  ClusterPlan cull;                   // the five kernels in front, exactly as mip_cull_clusters plans them
  uint32_t test_blocks;               // the triangle test's grid
  uint32_t write_blocks;              // the write kernel's grid
  uint32_t command_blocks;            // the commands kernel's grid
  unsigned long long triangle_words;  // 8 bytes each: the triangle word of a work item
  unsigned long long item_prefixes;   // 4 bytes each: the exclusive prefix of every work item, and the entry at W
  unsigned long long word_totals;     // 4 bytes each: the surviving triangles of a survive word's 64 items
  unsigned long long item_tiles;      // 8 bytes each: a tile's surviving and tested triangles
  constexpr bool test_loops() const { return test_blocks == kClusterMaxBlocks; }
  // bytes per frame slot on top of mip_cull_clusters': 12 per work item of the bound, and 1/16 + 1/128 of a byte
  constexpr unsigned long long scratch_bytes() const { return 8ull * triangle_words + 4ull * item_prefixes + 4ull * word_totals + 8ull * item_tiles; }
};
constexpr ClusterTrianglePlan plan_cluster_triangles(uint32_t n, unsigned long long bound) {
  ClusterTrianglePlan p{};
  p.cull = plan_cluster_cull(n, bound);
  p.test_blocks = p.cull.cull_blocks;
  p.write_blocks = p.cull.cull_blocks;
  p.command_blocks = p.cull.head_blocks;
  p.triangle_words = bound;
  p.item_prefixes = bound + 1ull;
  p.word_totals = p.cull.survive_words;
  const unsigned long long tiles = (bound + kClusterItemTile - 1u) / kClusterItemTile;
  p.item_tiles = tiles < 1u ? 1u : tiles;
  return p;
}

}  // namespace mip
