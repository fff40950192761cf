// cluster_views_plan.hpp — the arithmetic of cluster culling for several views in one call (mip_cull_clusters_views;
// extension, not reference behaviour) that is not a kernel: the scratch a call takes, its grids and its launch list, a pure
// function of (N, the bound on W, n_views). The tiles, the block cap, the bound and the tile permutation are cluster_plan.hpp's:
// a work item is common to all views, so the item tiles and the head tiles are the plain call's; what a view adds is one
// plane of survive words, one row of head counts and one of survivor counts, and one grid row of the heads / commands
// kernels. Plain C++, no HIP: api_cluster.hip and cluster_views_kernel.hpp call it, tests/native/cluster_views_plan_check.cpp
// enumerates it on the CPU over its decision edges.
#pragma once

#include "cluster_plan.hpp"

namespace mip {

constexpr uint32_t kClusterMaxViews = 16;      // MIP_MAX_VIEWS: a view is a bit of an instance's 16-bit mask
constexpr uint32_t kClusterViewsLaunches = 7;  // whatever n_views

// The kernels of a call, in launch order.
enum class ClusterViewsKernel : uint32_t { count, scan, members, cull, heads, epilogue, commands };

struct ClusterViewsLaunch {
  ClusterViewsKernel kernel;
  uint32_t blocks_x;   // tiles (or the capped, looping grid)
  uint32_t blocks_y;   // views, for the kernels that take one view per grid row; else 1
};

struct ClusterViewsPlan {
  ClusterPlan one;                      // the tiles and grids of one view: plan_cluster_cull(n, bound)
  uint32_t n_views;
  unsigned long long word_planes;       // 1 + n_views: the start words, then the survive words of every view
  unsigned long long words;             // 8 bytes each: word_planes x one.survive_words; plane p starts at p x one.survive_words
  unsigned long long tile_rows;         // 4 bytes each, twice (heads, survivors): n_views x one.head_tiles; view v's row starts at v x one.head_tiles
  unsigned long long mask_entries;      // 2 bytes each: the view mask of every instance
  ClusterViewsLaunch launches[kClusterViewsLaunches];
  constexpr unsigned long long scratch_bytes_per_call() const { return 8ull * words + 8ull * tile_rows + 2ull * mask_entries; }
};

// 1 <= n_views <= kClusterMaxViews (the entry point refuses anything else); bound <= kClusterMaxWork.
constexpr ClusterViewsPlan plan_cluster_views(uint32_t n, unsigned long long bound, uint32_t n_views) {
  ClusterViewsPlan p{};
  p.one = plan_cluster_cull(n, bound);
  p.n_views = n_views;
  p.word_planes = 1ull + n_views;
  p.words = p.word_planes * p.one.survive_words;
  p.tile_rows = (unsigned long long)n_views * p.one.head_tiles;
  p.mask_entries = n;
  p.launches[0] = {ClusterViewsKernel::count, p.one.instance_tiles, 1u};
  p.launches[1] = {ClusterViewsKernel::scan, 1u, 1u};
  p.launches[2] = {ClusterViewsKernel::members, p.one.instance_tiles, 1u};
  p.launches[3] = {ClusterViewsKernel::cull, p.one.cull_blocks, 1u};       // the views are a loop inside: the box is built once
  p.launches[4] = {ClusterViewsKernel::heads, p.one.head_blocks, n_views};
  p.launches[5] = {ClusterViewsKernel::epilogue, n_views, 1u};             // one workgroup per view
  p.launches[6] = {ClusterViewsKernel::commands, p.one.head_blocks, n_views};
  return p;
}

}  // namespace mip
