// cluster_triangle_list_plan.hpp — the arithmetic of mip_list_cluster_triangles (per-triangle masks on the visible-cluster
// list; extension, not reference behaviour) that is not a kernel: the grids of the four kernels behind the list's word
// members, the scratch they take and the work-item count from which the test and write grids loop, all pure functions of the
// call's bound on W. Plain C++, no HIP: api_cluster.hip and cluster_triangle_list_kernel.hpp call it,
// tests/native/cluster_triangle_list_plan_check.cpp enumerates it on the CPU over its decision edges.
#pragma once

#include "cluster_list_plan.hpp"

namespace mip {

constexpr uint32_t kClusterTriangleListStats = 6;  // entries, surviving clusters, W, members, surviving triangles, triangles tested

// The bound from which the test and the write grid stop growing and loop over their item tiles: kClusterMaxBlocks tiles.
constexpr unsigned long long kClusterTriangleListLoopItems = (unsigned long long)kClusterMaxBlocks * kClusterItemTile;  // = 2 097 152

// What the call launches and allocates behind the front it shares with mip_list_clusters (count, scan, members, cull) and
// that call's word members. The test and the write kernel walk the cull kernel's item tiles, the count kernel the list tiles;
// all three grids are capped at kClusterMaxBlocks and loop.
struct ClusterTriangleListPlan {
  ClusterListPlan list;               // word_member, word_rank and list_tiles exactly as mip_list_clusters plans them
  uint32_t test_blocks;               // the triangle test's grid: item tiles
  uint32_t count_blocks;              // the count kernel's grid: list tiles
  uint32_t write_blocks;              // the write kernel's grid: item tiles
  unsigned long long triangle_words;  // 8 bytes each: the triangle word of a work item
  unsigned long long nonempty_words;  // 8 bytes each: the NON-EMPTY word of 64 work items
  unsigned long long item_tiles;      // 8 bytes each: an item tile's surviving and tested triangles
  uint32_t cluster_tiles;             // 4 bytes each: a list tile's surviving clusters
  constexpr bool test_loops() const { return test_blocks == kClusterMaxBlocks; }
  // bytes per frame slot on top of mip_cull_clusters': the list's 8 per 64 work items of the bound, 8 per work item, 8 per 64,
  // and the tile sums (8 per 1 024 and 4 + 4 per 16 384)
  constexpr unsigned long long scratch_bytes() const {
    return 8ull * list.words + 4ull * list.list_tiles + 8ull * triangle_words + 8ull * nonempty_words + 8ull * item_tiles + 4ull * cluster_tiles;
  }
};
constexpr ClusterTriangleListPlan plan_cluster_triangle_list(unsigned long long bound) {
  ClusterTriangleListPlan p{};
  p.list = plan_cluster_list(bound);
  p.test_blocks = p.list.write_blocks;
  p.count_blocks = p.list.word_blocks;
  p.write_blocks = p.list.write_blocks;
  p.triangle_words = bound;
  p.nonempty_words = p.list.words;
  const unsigned long long tiles = (bound + kClusterItemTile - 1u) / kClusterItemTile;
  p.item_tiles = tiles < 1u ? 1u : tiles;
  p.cluster_tiles = p.list.list_tiles;
  return p;
}

}  // namespace mip
