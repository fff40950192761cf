// cluster_list_plan.hpp — the arithmetic of mip_list_clusters (the visible-cluster list for one indirect draw; extension, not
// reference behaviour) that is not a kernel: the list tile, the grids and the scratch the list kernels take as a pure function
// of the bound on W, the index count of an entry, the words a member's first item lies in front of, and the member of a
// word's first item. Plain C++, no HIP: api_cluster.hip and cluster_list_kernel.hpp call it,
// tests/native/cluster_list_plan_check.cpp enumerates it on the CPU over its decision edges.
#pragma once

#include "cluster_plan.hpp"

namespace mip {

constexpr uint32_t kClusterListTileWords = 256;                       // survive words per tile of the word-member and count kernels: one per thread
constexpr uint32_t kClusterListTile = 64 * kClusterListTileWords;     // = 16 384 work items
constexpr uint32_t kClusterListDrawVertices = kClusterIndices;        // draw_args[0]: every entry is drawn with 192 vertices

MIP_CLUSTER_HD constexpr uint32_t cluster_list_tiles(uint32_t w) { return w / kClusterListTile + (w % kClusterListTile ? 1u : 0u); }

// index_count of the entry of cluster c of a level of T triangles (c < C): 192, or fewer in the last cluster
MIP_CLUSTER_HD constexpr uint32_t cluster_list_index_count(uint32_t c, uint32_t t) { return 3u * cluster_triangles(c, t); }

// The words whose first item belongs to a member with items [first, next), first < next: word k for lo <= k < hi, where
// first <= 64 k < next. Empty (lo == hi) for a member that lies inside one word behind the word's first item. word_member's
// definition member by member: the plan check holds cluster_list_word_member (the kernel's search, per word) against it.
struct ClusterListWordRange {
  uint32_t lo, hi;
};
MIP_CLUSTER_HD constexpr ClusterListWordRange cluster_list_member_words(uint32_t first, uint32_t next) {
  return {first / 64u + (first % 64u ? 1u : 0u), next / 64u + (next % 64u ? 1u : 0u)};
}

// word_member[k]: the member m with member_first[m] <= 64 k < member_first[m + 1], for 64 k < W = member_first[members]
// (members >= 1, member_first[0] = 0, strictly increasing; W < 2^32, so 64 k does not wrap).
MIP_CLUSTER_HD inline uint32_t cluster_list_word_member(const uint32_t* member_first, uint32_t members, uint32_t k) {
  const uint32_t item = k * 64u;
  uint32_t lo = 0, hi = members;
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (member_first[mid] <= item) lo = mid; else hi = mid;
  }
  return lo;
}

// What the list tail launches and allocates behind the front mip_cull_clusters shares with it (count, scan, members, cull):
// a pure function of the bound on W (nothing here depends on N). The looping grids are capped at kClusterMaxBlocks, as the front's.
struct ClusterListPlan {
  uint32_t word_blocks;      // the word-member and count kernels' grid: list tiles
  uint32_t write_blocks;     // the write kernel's grid: the cull kernel's item tiles
  unsigned long long words;  // word_member and word_rank: 4 bytes each per 64 work items of the bound
  uint32_t list_tiles;       // rows of the tile totals
};
constexpr ClusterListPlan plan_cluster_list(unsigned long long bound) {
  ClusterListPlan p{};
  const unsigned long long item_tiles = (bound + kClusterItemTile - 1u) / kClusterItemTile;
  const unsigned long long list_tiles = (bound + kClusterListTile - 1u) / kClusterListTile;
  p.word_blocks = list_tiles < 1u ? 1u : list_tiles < kClusterMaxBlocks ? (uint32_t)list_tiles : kClusterMaxBlocks;
  p.write_blocks = item_tiles < 1u ? 1u : item_tiles < kClusterMaxBlocks ? (uint32_t)item_tiles : kClusterMaxBlocks;
  p.words = (bound + 63u) / 64u;
  p.list_tiles = list_tiles < 1u ? 1u : (uint32_t)list_tiles;
  return p;
}

}  // namespace mip
