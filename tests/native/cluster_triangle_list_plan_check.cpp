// cluster_triangle_list_plan_check.cpp — enumerates cluster_triangle_list_plan.hpp (renderer_amd/csrc) over its decision
// edges: the grids of the test, count and write kernels around the sizes at which they stop growing and loop, the front and
// the word members planned exactly as mip_list_clusters plans them, and the scratch a call takes — every word a kernel
// touches for a W within the bound lies inside it, and the whole is the list's words, 8 bytes per item, 8 per 64 items and
// the tile sums. Plain C++, no HIP: built by tests/test_cluster_triangle_list_restatement.py with g++
// -fsanitize=address,undefined. Prints "CLUSTER TRIANGLE LIST PLAN OK <checks>". With the argument `sizes` it prints, as one
// JSON line, the tiles and the work items at which each looping grid stops growing: the GPU tests read their edges from it.
#include "../../renderer_amd/csrc/cluster_triangle_list_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>

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

// the largest W (= the call's bound) whose tiles a grid of the plan still takes one each: above it the grid loops
template <class Loops>
static unsigned long long largest_without_loop(Loops loops) {
  unsigned long long lo = 0, hi = kClusterMaxWork;  // !loops(lo), loops(hi)
  while (hi - lo > 1ull) {
    const unsigned long long mid = lo + (hi - lo) / 2ull;
    if (loops(plan_cluster_triangle_list(mid), (uint32_t)mid)) hi = mid; else lo = mid;
  }
  return lo;
}

int main(int argc, char**) {
  const unsigned long long test_cap = largest_without_loop([](const ClusterTriangleListPlan& p, uint32_t w) { return cluster_item_tiles(w) > p.test_blocks; });
  const unsigned long long write_cap = largest_without_loop([](const ClusterTriangleListPlan& p, uint32_t w) { return cluster_item_tiles(w) > p.write_blocks; });
  const unsigned long long count_cap = largest_without_loop([](const ClusterTriangleListPlan& p, uint32_t w) { return cluster_list_tiles(w) > p.count_blocks; });
  if (argc > 1) {
    std::printf("{\"item_tile\": %u, \"list_tile\": %u, \"max_blocks\": %u, \"test_grid_cap\": %llu, \"write_grid_cap\": %llu, \"count_grid_cap\": %llu}\n",
                kClusterItemTile, kClusterListTile, kClusterMaxBlocks, test_cap, write_cap, count_cap);
    return 0;
  }
  static_assert(plan_cluster_triangle_list(1024).test_blocks == 1 && plan_cluster_triangle_list(1025).test_blocks == 2, "usable at compile time");
  static_assert(plan_cluster_triangle_list(16384).count_blocks == 1 && plan_cluster_triangle_list(16385).count_blocks == 2, "usable at compile time");

  CHECK(test_cap == kClusterTriangleListLoopItems && write_cap == test_cap, "the test and write grids take a tile each up to %llu items", test_cap);
  CHECK(count_cap == (unsigned long long)kClusterMaxBlocks * kClusterListTile, "the count grid takes a tile each up to %llu items", count_cap);
  const unsigned long long test_from = (unsigned long long)(kClusterMaxBlocks - 1u) * kClusterItemTile + 1ull;  // the bound from which the grid is at its cap
  for (unsigned long long edge : {1ull, 64ull, (unsigned long long)kClusterItemTile, (unsigned long long)kClusterListTile, test_from, test_cap,
                                  (unsigned long long)(kClusterMaxBlocks - 1u) * kClusterListTile + 1ull, count_cap, 1ull << 31, kClusterMaxWork - 1ull})
    for (unsigned long long bound = edge > 2ull ? edge - 2ull : 0ull; bound <= edge + 2ull && bound <= kClusterMaxWork; ++bound) {
      const ClusterTriangleListPlan p = plan_cluster_triangle_list(bound);
      const ClusterListPlan l = plan_cluster_list(bound);
      const unsigned long long item_tiles = (bound + kClusterItemTile - 1ull) / kClusterItemTile, list_tiles = (bound + kClusterListTile - 1ull) / kClusterListTile;
      CHECK(p.list.word_blocks == l.word_blocks && p.list.write_blocks == l.write_blocks && p.list.words == l.words && p.list.list_tiles == l.list_tiles,
            "bound %llu: the word members are planned as mip_list_clusters plans them", bound);
      CHECK(p.test_blocks >= 1u && p.test_blocks <= kClusterMaxBlocks && p.test_blocks == (item_tiles < 1ull ? 1ull : item_tiles < kClusterMaxBlocks ? item_tiles : kClusterMaxBlocks),
            "bound %llu: %u test blocks", bound, p.test_blocks);
      CHECK(p.write_blocks == p.test_blocks, "bound %llu: %u write blocks", bound, p.write_blocks);
      CHECK(p.count_blocks >= 1u && p.count_blocks == (list_tiles < 1ull ? 1ull : list_tiles < kClusterMaxBlocks ? list_tiles : kClusterMaxBlocks),
            "bound %llu: %u count blocks", bound, p.count_blocks);
      CHECK(p.test_loops() == (bound >= test_from), "bound %llu: loops %d", bound, (int)p.test_loops());
      // the scratch: every W within the bound touches only what the plan holds
      for (unsigned long long w : {0ull, 1ull, bound / 2ull, bound > 0ull ? bound - 1ull : 0ull, bound}) {
        if (!cluster_work_fits(w, bound)) continue;
        const uint32_t w32 = (uint32_t)w;
        CHECK(w <= p.triangle_words, "W %llu: a triangle word per item", w);
        CHECK(cluster_survive_words(w32) <= p.nonempty_words && cluster_survive_words(w32) <= p.list.words, "W %llu: a non-empty word, a member and a rank per 64 items", w);
        CHECK(cluster_item_tiles(w32) <= p.item_tiles, "W %llu: a row per item tile", w);
        CHECK(cluster_list_tiles(w32) <= p.cluster_tiles && cluster_list_tiles(w32) <= p.list.list_tiles, "W %llu: a row per list tile", w);
        // the write kernel reads list_tiles[word / 256] for every word below the survive words of W
        if (w) CHECK((cluster_survive_words(w32) - 1u) / kClusterListTileWords < p.list.list_tiles, "W %llu: the last word's tile", w);
      }
      // the list's words, 8 bytes per item, 8 per 64 items, the tile sums
      const unsigned long long words = (bound + 63ull) / 64ull;
      const unsigned long long want = 8ull * words + 8ull * bound + 8ull * words + 8ull * (item_tiles < 1ull ? 1ull : item_tiles) + 8ull * (list_tiles < 1ull ? 1ull : list_tiles);
      CHECK(p.scratch_bytes() == want, "bound %llu: %llu bytes of scratch, not %llu", bound, p.scratch_bytes(), want);
      CHECK(p.scratch_bytes() >= 8ull * bound && p.scratch_bytes() <= 8ull * bound + bound / 4ull + bound / 64ull + 64ull, "bound %llu: %llu bytes of scratch", bound, p.scratch_bytes());
    }
  std::printf("CLUSTER TRIANGLE LIST PLAN OK %llu\n", checks);
  return 0;
}
