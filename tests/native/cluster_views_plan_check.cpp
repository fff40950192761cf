// cluster_views_plan_check.cpp — enumerates cluster_views_plan.hpp (renderer_amd/csrc) over its decision edges: 1 .. 16 views,
// bounds around the survive word, the item tile, the head tile, the 2 048-workgroup cap of both looping grids and W around
// 2^32; the scratch sizes, the grids and the launch list of every plan, and that whatever W the device finds under the bound has
// a word in every plane and a row entry for every view. Plain C++, no HIP: built by tests/test_cluster_views_restatement.py
// with g++ -fsanitize=address,undefined. Prints "CLUSTER VIEWS PLAN OK <checks>". With the argument `sizes` it prints the
// plan's tile sizes, the block cap and the view limit as one JSON line instead: the GPU tests read their edges from it.
#include "../../renderer_amd/csrc/cluster_views_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace mip;

#define CHECK(cond, ...)                                            \
  do {                                                              \
    ++checks;                                                       \
    if (!(cond)) {                                                  \
      std::printf("FAILED %s:%d %s — ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                                     \
      std::printf("\n");                                            \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

static unsigned long long checks = 0;

int main(int argc, char**) {
  if (argc > 1) {
    std::printf("{\"instance_tile\": %u, \"item_tile\": %u, \"head_tile\": %u, \"max_blocks\": %u, \"max_views\": %u, \"launches\": %u}\n",
                kClusterInstanceTile, kClusterItemTile, kClusterHeadTile, kClusterMaxBlocks, kClusterMaxViews, kClusterViewsLaunches);
    return 0;
  }
  static_assert(plan_cluster_views(1, 1, 1).words == 2, "usable at compile time: a start word and one view's survive word");
  static_assert(kClusterViewsLaunches == 7, "the launches do not depend on n_views");

  const unsigned long long cull_cap = (unsigned long long)kClusterMaxBlocks * kClusterItemTile, head_cap = (unsigned long long)kClusterMaxBlocks * kClusterHeadTile;
  const unsigned long long bounds[] = {0ull, 1ull, 63ull, 64ull, 65ull, 1023ull, 1024ull, 1025ull, 16383ull, 16384ull, 16385ull, cull_cap - 1, cull_cap, cull_cap + 1,
                                       head_cap - 1, head_cap, head_cap + 1, (1ull << 32) - 65ull, (1ull << 32) - 64ull, (1ull << 32) - 2ull, kClusterMaxWork};
  const ClusterViewsKernel order[kClusterViewsLaunches] = {ClusterViewsKernel::count, ClusterViewsKernel::scan, ClusterViewsKernel::members,
                                                           ClusterViewsKernel::cull, ClusterViewsKernel::heads, ClusterViewsKernel::epilogue,
                                                           ClusterViewsKernel::commands};
  for (uint32_t views = 1; views <= kClusterMaxViews; ++views)
    for (uint32_t n : {1u, 1023u, 1024u, 1025u, 2049u, 1u << 20, 0xFFFFFFFFu})
      for (unsigned long long bound : bounds) {
        const ClusterViewsPlan p = plan_cluster_views(n, bound, views);
        const ClusterPlan one = plan_cluster_cull(n, bound);
        // the tiles and grids of one view are the plain call's
        CHECK(p.one.instance_tiles == one.instance_tiles && p.one.cull_blocks == one.cull_blocks && p.one.head_blocks == one.head_blocks &&
                  p.one.survive_words == one.survive_words && p.one.head_tiles == one.head_tiles,
              "views %u n %u bound %llu: the plain plan", views, n, bound);
        CHECK(p.n_views == views && p.word_planes == 1ull + views, "views %u: %llu planes", views, p.word_planes);
        // scratch: (1 + n_views) x 8 B per 64 work items of the bound, 2 B per instance, two rows of head tiles per view
        CHECK(p.words == (1ull + views) * ((bound + 63ull) / 64ull), "views %u bound %llu: %llu words", views, bound, p.words);
        CHECK(p.tile_rows == (unsigned long long)views * one.head_tiles && p.mask_entries == n, "views %u bound %llu: rows", views, bound);
        CHECK(p.scratch_bytes_per_call() == 8ull * p.words + 8ull * p.tile_rows + 2ull * n, "views %u bound %llu: bytes", views, bound);
        CHECK(p.words < (1ull << 31) && 8ull * p.words < (1ull << 34), "views %u bound %llu: the planes stay far inside a 64-bit byte count", views, bound);
        // whatever W <= bound the device finds: every plane has its words, every row its tiles
        if (bound <= kClusterMaxWork) {
          const uint32_t w = (uint32_t)bound;
          CHECK(cluster_survive_words(w) <= p.one.survive_words && cluster_head_tiles(w) <= p.one.head_tiles, "views %u bound %llu: room for every W", views, bound);
          // the last word of the last plane and the last entry of the last row lie inside the allocations
          if (w) {
            CHECK((unsigned long long)views * p.one.survive_words + (cluster_survive_words(w) - 1u) < p.words, "views %u bound %llu: the last word", views, bound);
            CHECK((unsigned long long)(views - 1u) * p.one.head_tiles + (cluster_head_tiles(w) - 1u) < p.tile_rows, "views %u bound %llu: the last row entry", views, bound);
          }
        }
        // the launch list: seven launches in order, the views a grid row of heads and commands only, every grid within the cap
        for (uint32_t k = 0; k < kClusterViewsLaunches; ++k) {
          const ClusterViewsLaunch& l = p.launches[k];
          CHECK(l.kernel == order[k], "views %u: launch %u", views, k);
          const bool per_view = l.kernel == ClusterViewsKernel::heads || l.kernel == ClusterViewsKernel::commands;
          CHECK(l.blocks_y == (per_view ? views : 1u) && l.blocks_x >= 1u, "views %u: launch %u rows %u", views, k, l.blocks_y);
          const bool looping = per_view || l.kernel == ClusterViewsKernel::cull;
          if (looping) CHECK(l.blocks_x <= kClusterMaxBlocks, "views %u bound %llu: launch %u has %u blocks", views, bound, k, l.blocks_x);
          if (l.kernel == ClusterViewsKernel::scan) CHECK(l.blocks_x == 1u, "one workgroup");
          if (l.kernel == ClusterViewsKernel::epilogue) CHECK(l.blocks_x == views, "one workgroup per view");
          if (l.kernel == ClusterViewsKernel::count || l.kernel == ClusterViewsKernel::members) CHECK(l.blocks_x == one.instance_tiles, "instance tiles");
          if (l.kernel == ClusterViewsKernel::cull) CHECK(l.blocks_x == one.cull_blocks, "the cull grid");
          if (per_view) CHECK(l.blocks_x == one.head_blocks, "the head grid");
        }
        // where the grids stop growing
        const unsigned long long item_tiles = (bound + kClusterItemTile - 1) / kClusterItemTile, head_tiles = (bound + kClusterHeadTile - 1) / kClusterHeadTile;
        CHECK(p.launches[3].blocks_x == (item_tiles < 1 ? 1u : item_tiles < kClusterMaxBlocks ? item_tiles : kClusterMaxBlocks), "bound %llu: cull grid", bound);
        CHECK(p.launches[4].blocks_x == (head_tiles < 1 ? 1u : head_tiles < kClusterMaxBlocks ? head_tiles : kClusterMaxBlocks), "bound %llu: head grid", bound);
      }
  // W around 2^32: the decision the scan makes, under the largest bound a plan is made for
  for (unsigned long long w : {(1ull << 32) - 2ull, (1ull << 32) - 1ull, 1ull << 32, (1ull << 32) + 1ull, 1ull << 40})
    CHECK(cluster_work_fits(w, cluster_work_bound(0xFFFFFFFFu, 0xFFFFFFFFu, 0)) == (w < (1ull << 32)), "W %llu", w);
  // the tile permutation every new looping grid uses is cluster_plan.hpp's: a bijection at the tile counts of the edges above
  for (uint32_t order_kind : {kClusterOrderReverse, kClusterOrderScramble})
    for (uint32_t tiles : {1u, 2u, kClusterMaxBlocks - 1u, kClusterMaxBlocks, kClusterMaxBlocks + 1u}) {
      std::vector<unsigned char> seen(tiles, 0);
      for (uint32_t t = 0; t < tiles; ++t) {
        const uint32_t to = cluster_permute_tile(t, tiles, order_kind);
        CHECK(to < tiles && !seen[to], "order %u, %u tiles: tile %u -> %u", order_kind, tiles, t, to);
        seen[to] = 1;
      }
    }
  std::printf("CLUSTER VIEWS PLAN OK %llu\n", checks);
  return 0;
}
