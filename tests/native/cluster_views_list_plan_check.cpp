// cluster_views_list_plan_check.cpp — enumerates cluster_views_list_plan.hpp (renderer_amd/csrc) over its decision edges:
// 1 .. 16 views, bounds around the survive word, the item tile, the list tile, the 2 048-workgroup cap of both looping grids
// and W around 2^32; the scratch sizes, the grids and the launch list of every plan, that whatever W the device finds under
// the bound has a word in every plane and an entry in every row, and where n_views x entry_stride stops fitting 32 bits. Plain
// C++, no HIP: built by tests/test_cluster_views_list_restatement.py with g++ -fsanitize=address,undefined. Prints
// "CLUSTER VIEWS LIST PLAN OK <checks>". With the argument `sizes` it prints the plan's tile sizes, the block cap and the view
// limit as one JSON line instead: the GPU tests read their edges from it.
#include "../../renderer_amd/csrc/cluster_views_list_plan.hpp"

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
    std::printf("{\"instance_tile\": %u, \"item_tile\": %u, \"list_tile\": %u, \"max_blocks\": %u, \"max_views\": %u, \"launches\": %u}\n",
                kClusterInstanceTile, kClusterItemTile, kClusterListTile, kClusterMaxBlocks, kClusterMaxViews, kClusterViewsListLaunches);
    return 0;
  }
  static_assert(plan_cluster_views_list(1, 65, 3).rank_words == 6 && plan_cluster_views_list(1, 65, 3).member_words == 2, "usable at compile time");
  static_assert(kClusterViewsListLaunches == 8, "the launches do not depend on n_views");

  const unsigned long long write_cap = (unsigned long long)kClusterMaxBlocks * kClusterItemTile, list_cap = (unsigned long long)kClusterMaxBlocks * kClusterListTile;
  const unsigned long long bounds[] = {0ull, 1ull, 63ull, 64ull, 65ull, 1023ull, 1024ull, 1025ull, 16383ull, 16384ull, 16385ull, write_cap - 1, write_cap, write_cap + 1,
                                       list_cap - 1, list_cap, list_cap + 1, (1ull << 32) - 65ull, (1ull << 32) - 64ull, (1ull << 32) - 2ull, kClusterMaxWork};
  const ClusterViewsListKernel order[kClusterViewsListLaunches] = {ClusterViewsListKernel::count, ClusterViewsListKernel::scan, ClusterViewsListKernel::members,
                                                                   ClusterViewsListKernel::cull, ClusterViewsListKernel::word_members, ClusterViewsListKernel::list_count,
                                                                   ClusterViewsListKernel::list_epilogue, ClusterViewsListKernel::list_write};
  for (uint32_t views = 1; views <= kClusterMaxViews; ++views)
    for (uint32_t n : {1u, 1023u, 1024u, 1025u, 2049u, 1u << 20, 0xFFFFFFFFu})
      for (unsigned long long bound : bounds) {
        const ClusterViewsListPlan p = plan_cluster_views_list(n, bound, views);
        const ClusterViewsPlan front = plan_cluster_views(n, bound, views);
        const ClusterListPlan list = plan_cluster_list(bound);
        // the front is the several-view call's, the tiles of the tail are the one-view list's
        CHECK(p.front.words == front.words && p.front.tile_rows == front.tile_rows && p.front.one.survive_words == front.one.survive_words &&
                  p.front.one.instance_tiles == front.one.instance_tiles && p.front.one.cull_blocks == front.one.cull_blocks,
              "views %u n %u bound %llu: the front", views, n, bound);
        CHECK(p.list.word_blocks == list.word_blocks && p.list.write_blocks == list.write_blocks && p.list.words == list.words && p.list.list_tiles == list.list_tiles,
              "views %u bound %llu: the list tail of one view", views, bound);
        CHECK(p.n_views == views, "views %u", views);
        // scratch: word_member ONE plane of 4 B per 64 work items of the bound, word_rank n_views planes, list_tiles n_views rows
        const unsigned long long words = (bound + 63ull) / 64ull;
        CHECK(p.member_words == words && p.rank_words == (unsigned long long)views * words, "views %u bound %llu: %llu + %llu words", views, bound, p.member_words,
              p.rank_words);
        CHECK(p.tile_rows == (unsigned long long)views * list.list_tiles, "views %u bound %llu: %llu row entries", views, bound, p.tile_rows);
        CHECK(p.list_scratch_bytes() == 4ull * ((1ull + views) * words + (unsigned long long)views * list.list_tiles), "views %u bound %llu: bytes", views, bound);
        CHECK(p.rank_words < (1ull << 31), "views %u bound %llu: the planes stay far inside a 64-bit byte count", views, bound);
        // a plane of word ranks is as long as a plane of survive words: one index serves both
        CHECK(p.list.words == p.front.one.survive_words, "views %u bound %llu: %llu rank words, %llu survive words per plane", views, bound, p.list.words,
              (unsigned long long)p.front.one.survive_words);
        // whatever W <= bound the device finds: every plane has its words, every row its tiles, and the last ones lie inside
        if (bound <= kClusterMaxWork) {
          const uint32_t w = (uint32_t)bound;
          CHECK(cluster_survive_words(w) <= p.list.words && cluster_list_tiles(w) <= p.list.list_tiles, "views %u bound %llu: room for every W", views, bound);
          if (w) {
            CHECK(cluster_survive_words(w) - 1u < p.member_words, "views %u bound %llu: the last member word", views, bound);
            CHECK((unsigned long long)(views - 1u) * p.list.words + (cluster_survive_words(w) - 1u) < p.rank_words, "views %u bound %llu: the last rank word", views, bound);
            CHECK((unsigned long long)(views - 1u) * p.list.list_tiles + (cluster_list_tiles(w) - 1u) < p.tile_rows, "views %u bound %llu: the last row entry", views, bound);
            // the write kernel's word -> list tile: an item tile lies inside one list tile
            CHECK((cluster_survive_words(w) - 1u) / kClusterListTileWords == cluster_list_tiles(w) - 1u, "bound %llu: the last word's list tile", bound);
          }
        }
        // the launch list: eight launches in order; the views a grid row of the list count only; every looping grid within the cap
        for (uint32_t k = 0; k < kClusterViewsListLaunches; ++k) {
          const ClusterViewsListLaunch& l = p.launches[k];
          CHECK(l.kernel == order[k], "views %u: launch %u", views, k);
          const bool per_view = l.kernel == ClusterViewsListKernel::list_count;
          CHECK(l.blocks_y == (per_view ? views : 1u) && l.blocks_x >= 1u, "views %u: launch %u rows %u", views, k, l.blocks_y);
          if (k < 4u) CHECK(l.blocks_x == front.launches[k].blocks_x && l.blocks_y == front.launches[k].blocks_y, "views %u: launch %u is the front's", views, k);
          if (l.kernel == ClusterViewsListKernel::cull || k >= 4u) CHECK(l.blocks_x <= kClusterMaxBlocks, "views %u bound %llu: launch %u has %u blocks", views, bound, k, l.blocks_x);
          if (l.kernel == ClusterViewsListKernel::word_members || per_view) CHECK(l.blocks_x == list.word_blocks, "the list-tile grid");
          if (l.kernel == ClusterViewsListKernel::list_epilogue) CHECK(l.blocks_x == views, "one workgroup per view");
          if (l.kernel == ClusterViewsListKernel::list_write) CHECK(l.blocks_x == list.write_blocks && l.blocks_x == front.one.cull_blocks, "the write grid is the cull kernel's");
        }
        // where the grids stop growing
        const unsigned long long item_tiles = (bound + kClusterItemTile - 1) / kClusterItemTile, list_tiles = (bound + kClusterListTile - 1) / kClusterListTile;
        CHECK(p.launches[7].blocks_x == (item_tiles < 1 ? 1u : item_tiles < kClusterMaxBlocks ? item_tiles : kClusterMaxBlocks), "bound %llu: write grid", bound);
        CHECK(p.launches[5].blocks_x == (list_tiles < 1 ? 1u : list_tiles < kClusterMaxBlocks ? list_tiles : kClusterMaxBlocks), "bound %llu: count grid", bound);
      }
  // n_views x entry_stride: refused from 2^32 on; below it every view's first entry, and its last, fit 32 bits
  for (uint32_t views = 1; views <= kClusterMaxViews; ++views) {
    const unsigned long long edge = ((1ull << 32) + views - 1ull) / views;  // the smallest stride that does not fit
    for (unsigned long long stride : {0ull, 1ull, edge - 2ull, edge - 1ull, edge, edge + 1ull, 0xFFFFFFFFull}) {
      if (stride > 0xFFFFFFFFull || (long long)stride < 0) continue;
      const bool fits = cluster_views_list_fits(views, (uint32_t)stride);
      CHECK(fits == (views * stride < (1ull << 32)), "views %u stride %llu", views, stride);
      if (fits && stride) CHECK(cluster_views_list_first(views - 1u, (uint32_t)stride) + stride - 1ull <= 0xFFFFFFFFull, "views %u stride %llu: the last entry", views, stride);
      CHECK(cluster_views_list_first(views - 1u, (uint32_t)stride) == (views - 1ull) * stride, "views %u stride %llu: the first entry", views, stride);
    }
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
  std::printf("CLUSTER VIEWS LIST PLAN OK %llu\n", checks);
  return 0;
}
