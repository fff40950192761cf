// cluster_list_phase_plan.hpp — the arithmetic of the two-phase visible-cluster list (mip_list_clusters_phase; extension, not
// reference behaviour) that is not a kernel: the launch list of each phase, the grids, the scratch — the candidates' tile row
// and the two scalars the epilogue leaves for the write kernel included — and the room behind an entry base. The front's
// tiles are mip_cull_clusters_phase's (cluster_plan.hpp), the tail's are mip_list_clusters' (cluster_list_plan.hpp). Plain
// C++, no HIP: api_cluster.hip and cluster_list_phase_kernel.hpp call it, tests/native/cluster_list_phase_plan_check.cpp
// enumerates it on the CPU over its decision edges.
#pragma once

#include "cluster_list_plan.hpp"

namespace mip {

constexpr uint32_t kClusterListPhaseLaunches = 8;  // either phase

// The kernels of a call, in launch order. word_members stands in front of the front: it needs member_first alone, and the
// front locates its items through word_member.
enum class ClusterListPhaseKernel : uint32_t { count, scan, members, word_members, front, list_count, list_epilogue, list_write };

// phase_scalars[]: what the epilogue leaves for the write kernel
constexpr uint32_t kClusterListPhaseScBase = 0;   // b = *entry_base, or 0
constexpr uint32_t kClusterListPhaseScRoom = 1;   // entry_capacity - min(b, entry_capacity)
constexpr uint32_t kClusterListPhaseScWords = 2;

struct ClusterListPhaseLaunch {
  ClusterListPhaseKernel kernel;
  uint32_t blocks;   // tiles, the capped looping grid, or 1
};

struct ClusterListPhasePlan {
  ClusterPlan front;                    // instance tiles, the item tiles of the cull / retest grid: plan_cluster_cull(n, bound)
  ClusterListPlan list;                 // the list tiles and the write grid: plan_cluster_list(bound)
  bool first;                           // FIRST: the cull in the front's place and the candidates' row; SECOND: the retest
  unsigned long long survive_words;     // 16 bytes each (the front's own scratch, shared with the command calls of the slot)
  unsigned long long member_words;      // word_member, 4 bytes each
  unsigned long long rank_words;        // word_rank, 4 bytes each
  uint32_t tile_rows;                   // list_tiles, 4 bytes each
  uint32_t candidate_rows;              // FIRST: the popcounts of the record's words per list tile, 4 bytes each; SECOND: 0
  uint32_t scalar_words;                // b and room
  ClusterListPhaseLaunch launches[kClusterListPhaseLaunches];
  // on top of the front's (16 bytes per 64 work items and the per-instance columns)
  constexpr unsigned long long list_scratch_bytes() const { return 4ull * (member_words + rank_words + tile_rows + candidate_rows + scalar_words); }
};

// The entries a list that starts at entry b may write into a buffer of `capacity` entries counted from entry 0.
MIP_CLUSTER_HD constexpr uint32_t cluster_list_phase_room(uint32_t b, uint32_t capacity) { return capacity - (b < capacity ? b : capacity); }
// entry_count of a list with `survivors` survivors behind base b
MIP_CLUSTER_HD constexpr uint32_t cluster_list_phase_count(uint32_t survivors, uint32_t b, uint32_t capacity) {
  return survivors < cluster_list_phase_room(b, capacity) ? survivors : cluster_list_phase_room(b, capacity);
}

// bound: the caller's or the library's, with the work items the record has words for folded in (cluster_record_items).
constexpr ClusterListPhasePlan plan_cluster_list_phase(uint32_t n, unsigned long long bound, bool first) {
  ClusterListPhasePlan p{};
  p.front = plan_cluster_cull(n, bound);
  p.list = plan_cluster_list(bound);
  p.first = first;
  p.survive_words = p.front.survive_words;
  p.member_words = p.list.words;
  p.rank_words = p.list.words;
  p.tile_rows = p.list.list_tiles;
  p.candidate_rows = first ? p.list.list_tiles : 0u;
  p.scalar_words = kClusterListPhaseScWords;
  p.launches[0] = {ClusterListPhaseKernel::count, p.front.instance_tiles};
  p.launches[1] = {ClusterListPhaseKernel::scan, 1u};
  p.launches[2] = {ClusterListPhaseKernel::members, p.front.instance_tiles};
  p.launches[3] = {ClusterListPhaseKernel::word_members, p.list.word_blocks};
  p.launches[4] = {ClusterListPhaseKernel::front, first ? p.front.cull_blocks : p.front.retest_blocks};
  p.launches[5] = {ClusterListPhaseKernel::list_count, p.list.word_blocks};
  p.launches[6] = {ClusterListPhaseKernel::list_epilogue, 1u};
  p.launches[7] = {ClusterListPhaseKernel::list_write, p.list.write_blocks};
  return p;
}

}  // namespace mip
