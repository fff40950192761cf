// cluster_views_list_plan.hpp — the arithmetic of the visible-cluster lists for several views in one call
// (mip_list_clusters_views; extension, not reference behaviour) that is not a kernel: the launch list, the grids and the
// scratch, a pure function of (N, the bound on W, n_views). The front is mip_cull_clusters_views' first four launches
// (cluster_views_plan.hpp), the tiles of the tail are mip_list_clusters' (cluster_list_plan.hpp): a work item is common to all
// views, so word_member is one plane; what a view adds is one plane of word ranks and one row of list-tile counts. Plain C++,
// no HIP: api_cluster.hip and cluster_views_list_kernel.hpp call it, tests/native/cluster_views_list_plan_check.cpp enumerates
// it on the CPU over its decision edges.
#pragma once

#include "cluster_list_plan.hpp"
#include "cluster_views_plan.hpp"

namespace mip {

constexpr uint32_t kClusterViewsListLaunches = 8;  // whatever n_views

// The kernels of a call, in launch order: the several-view front, then the list tail.
enum class ClusterViewsListKernel : uint32_t { count, scan, members, cull, word_members, list_count, list_epilogue, list_write };

struct ClusterViewsListLaunch {
  ClusterViewsListKernel kernel;
  uint32_t blocks_x;   // tiles (or the capped, looping grid)
  uint32_t blocks_y;   // views, for the kernel that takes one view per grid row; else 1
};

struct ClusterViewsListPlan {
  ClusterViewsPlan front;               // the planes, rows and grids of mip_cull_clusters_views: plan_cluster_views(n, bound, n_views)
  ClusterListPlan list;                 // the tiles and grids of one view's list tail: plan_cluster_list(bound)
  uint32_t n_views;
  unsigned long long member_words;      // word_member, 4 bytes each: ONE plane of list.words, common to all views
  unsigned long long rank_words;        // word_rank, 4 bytes each: n_views x list.words; view v's plane starts at v x list.words
  unsigned long long tile_rows;         // list_tiles, 4 bytes each: n_views x list.list_tiles; view v's row starts at v x list.list_tiles
  ClusterViewsListLaunch launches[kClusterViewsListLaunches];
  // on top of front.scratch_bytes_per_call()
  constexpr unsigned long long list_scratch_bytes() const { return 4ull * (member_words + rank_words + tile_rows); }
};

// The first entry of view v: firstInstance of its draw. The entry point refuses n_views x entry_stride >= 2^32, so every
// view's first entry, and every entry index of the call, fits 32 bits.
MIP_CLUSTER_HD constexpr unsigned long long cluster_views_list_first(uint32_t v, uint32_t entry_stride) { return (unsigned long long)v * entry_stride; }
MIP_CLUSTER_HD constexpr bool cluster_views_list_fits(uint32_t n_views, uint32_t entry_stride) { return cluster_views_list_first(n_views, entry_stride) < (1ull << 32); }

// 1 <= n_views <= kClusterMaxViews (the entry point refuses anything else); bound <= kClusterMaxWork.
constexpr ClusterViewsListPlan plan_cluster_views_list(uint32_t n, unsigned long long bound, uint32_t n_views) {
  ClusterViewsListPlan p{};
  p.front = plan_cluster_views(n, bound, n_views);
  p.list = plan_cluster_list(bound);
  p.n_views = n_views;
  p.member_words = p.list.words;
  p.rank_words = (unsigned long long)n_views * p.list.words;
  p.tile_rows = (unsigned long long)n_views * p.list.list_tiles;
  for (uint32_t k = 0; k < 4u; ++k)  // count, scan, members, cull: the several-view call's own, in its order and with its grids
    p.launches[k] = {(ClusterViewsListKernel)k, p.front.launches[k].blocks_x, p.front.launches[k].blocks_y};
  p.launches[4] = {ClusterViewsListKernel::word_members, p.list.word_blocks, 1u};        // once for all views
  p.launches[5] = {ClusterViewsListKernel::list_count, p.list.word_blocks, n_views};      // grid row = view, as heads
  p.launches[6] = {ClusterViewsListKernel::list_epilogue, n_views, 1u};                   // one workgroup per view
  p.launches[7] = {ClusterViewsListKernel::list_write, p.list.write_blocks, 1u};          // the views are a loop inside: the locate is done once
  return p;
}

static_assert((uint32_t)ClusterViewsListKernel::count == (uint32_t)ClusterViewsKernel::count && (uint32_t)ClusterViewsListKernel::cull == (uint32_t)ClusterViewsKernel::cull,
              "the front's four kernels are numbered as the several-view call numbers them");

}  // namespace mip
