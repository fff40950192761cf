// cluster_triangle_plan_check.cpp — enumerates cluster_triangle_plan.hpp (renderer_amd/csrc) over its decision edges: the
// index-overflow decision around index_capacity and around 2^32 indices (no test with data reaches those), the grids of the
// test, write and commands kernels around the sizes at which they stop growing and loop, and the scratch a call takes — every
// word a kernel touches for a W within the bound lies inside it. Plain C++, no HIP: built by
// tests/test_cluster_triangle_restatement.py with g++ -fsanitize=address,undefined. Prints "CLUSTER TRIANGLE PLAN OK <checks>".
// With the argument `sizes` it prints, as one JSON line, the work items at which each looping grid stops growing: the GPU
// tests read their edges from it.
#include "../../renderer_amd/csrc/cluster_triangle_plan.hpp"

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
    if (loops(plan_cluster_triangles(1u, mid), (uint32_t)mid)) hi = mid; else lo = mid;
  }
  return lo;
}

int main(int argc, char**) {
  const unsigned long long test_cap = largest_without_loop([](const ClusterTrianglePlan& p, uint32_t w) { return cluster_item_tiles(w) > p.test_blocks; });
  const unsigned long long write_cap = largest_without_loop([](const ClusterTrianglePlan& p, uint32_t w) { return cluster_item_tiles(w) > p.write_blocks; });
  const unsigned long long command_cap = largest_without_loop([](const ClusterTrianglePlan& p, uint32_t w) { return cluster_head_tiles(w) > p.command_blocks; });
  if (argc > 1) {
    std::printf("{\"instance_tile\": %u, \"item_tile\": %u, \"head_tile\": %u, \"max_blocks\": %u, \"test_grid_cap\": %llu, \"write_grid_cap\": %llu, \"command_grid_cap\": %llu}\n",
                kClusterInstanceTile, kClusterItemTile, kClusterHeadTile, kClusterMaxBlocks, test_cap, write_cap, command_cap);
    return 0;
  }
  static_assert(cluster_triangle_index_fits(0, 0) && !cluster_triangle_index_fits(1, 2) && cluster_triangle_index_fits(1, 3), "usable at compile time");
  static_assert(plan_cluster_triangles(1, 1024).test_blocks == 1 && plan_cluster_triangles(1, 1025).test_blocks == 2, "usable at compile time");

  // the index-overflow decision: 3 x triangles within the capacity, and a 32-bit firstIndex
  for (unsigned long long tris = 0; tris <= 700ull; ++tris)
    for (unsigned long long cap = 0; cap <= 2200ull; ++cap)
      CHECK(cluster_triangle_index_fits(tris, (uint32_t)cap) == (3ull * tris <= cap), "%llu triangles, capacity %llu", tris, cap);
  const unsigned long long most = 0xFFFFFFFFull / 3ull;  // 1 431 655 765 triangles = 2^32 - 1 indices
  for (unsigned long long tris : {most - 1ull, most, most + 1ull, most + 2ull, 1ull << 31, (1ull << 32) - 1ull, 1ull << 32, (1ull << 32) + 1ull,
                                  (1ull << 32) / 3ull * 2ull, 1ull << 33, 1ull << 62, 0xFFFFFFFFFFFFFFFFull / 3ull, 0xFFFFFFFFFFFFFFFFull / 3ull + 1ull,
                                  0xFFFFFFFFFFFFFFFFull})
    for (uint32_t cap : {0u, 2u, 3u, 0x7FFFFFFFu, 0xFFFFFFFCu, 0xFFFFFFFDu, 0xFFFFFFFEu, 0xFFFFFFFFu}) {
      const bool want = tris <= most && 3ull * tris <= cap;  // (tris <= most: the product does not wrap)
      CHECK(cluster_triangle_index_fits(tris, cap) == want, "%llu triangles, capacity %u", tris, cap);
      if (cluster_triangle_index_fits(tris, cap)) CHECK(3ull * tris < (1ull << 32) && (tris == 0ull || 3ull * (tris - 1ull) + 2ull < cap), "%llu triangles: the last index is inside", tris);
    }
  CHECK(cluster_triangle_index_fits(most, 0xFFFFFFFFu) && !cluster_triangle_index_fits(most + 1ull, 0xFFFFFFFFu), "the largest stream");

  // the grids: the cull kernel's item tiles and the heads kernel's head tiles, capped; they loop from the sizes `sizes` prints
  CHECK(test_cap == (unsigned long long)kClusterMaxBlocks * kClusterItemTile && write_cap == test_cap, "the test grid takes a tile each up to %llu items", test_cap);
  CHECK(command_cap == (unsigned long long)kClusterMaxBlocks * kClusterHeadTile, "the command grid takes a tile each up to %llu items", command_cap);
  const unsigned long long test_from = (unsigned long long)(kClusterMaxBlocks - 1u) * kClusterItemTile + 1ull;  // the bound from which the grid is at its cap
  for (unsigned long long edge : {1ull, 64ull, (unsigned long long)kClusterItemTile, (unsigned long long)kClusterHeadTile, test_from, test_cap,
                                  (unsigned long long)(kClusterMaxBlocks - 1u) * kClusterHeadTile + 1ull, command_cap, 1ull << 31, kClusterMaxWork - 1ull})
    for (unsigned long long bound = edge > 2ull ? edge - 2ull : 0ull; bound <= edge + 2ull && bound <= kClusterMaxWork; ++bound)
      for (uint32_t n : {1u, 1024u, 1025u, 1u << 20}) {
        const ClusterTrianglePlan p = plan_cluster_triangles(n, bound);
        const ClusterPlan c = plan_cluster_cull(n, bound);
        const unsigned long long item_tiles = (bound + kClusterItemTile - 1ull) / kClusterItemTile, head_tiles = (bound + kClusterHeadTile - 1ull) / kClusterHeadTile;
        CHECK(p.cull.cull_blocks == c.cull_blocks && p.cull.head_blocks == c.head_blocks && p.cull.survive_words == c.survive_words &&
              p.cull.instance_tiles == c.instance_tiles && p.cull.head_tiles == c.head_tiles, "bound %llu: the kernels in front are planned as mip_cull_clusters plans them", bound);
        CHECK(p.test_blocks >= 1u && p.test_blocks <= kClusterMaxBlocks && p.test_blocks == (item_tiles < 1ull ? 1ull : item_tiles < kClusterMaxBlocks ? item_tiles : kClusterMaxBlocks),
              "bound %llu: %u test blocks", bound, p.test_blocks);
        CHECK(p.write_blocks == p.test_blocks, "bound %llu: %u write blocks", bound, p.write_blocks);
        CHECK(p.command_blocks >= 1u && p.command_blocks == (head_tiles < 1ull ? 1ull : head_tiles < kClusterMaxBlocks ? head_tiles : kClusterMaxBlocks),
              "bound %llu: %u command blocks", bound, p.command_blocks);
        CHECK(p.test_loops() == (bound >= test_from), "bound %llu: loops %d", bound, (int)p.test_loops());
        // the scratch: every W within the bound touches only what the plan holds
        for (unsigned long long w : {0ull, 1ull, bound / 2ull, bound}) {
          if (!cluster_work_fits(w, bound)) continue;
          CHECK(w <= p.triangle_words, "W %llu: a triangle word per item", w);
          CHECK(w + 1ull <= p.item_prefixes, "W %llu: a prefix per item and the entry at W", w);
          CHECK(cluster_survive_words((uint32_t)w) <= p.word_totals, "W %llu: a total per survive word", w);
          CHECK(cluster_item_tiles((uint32_t)w) <= p.item_tiles, "W %llu: a row per item tile", w);
          // a tile's words: the write kernel reads kClusterTriangleTileWords totals per tile, below the survive words of W
          CHECK((unsigned long long)cluster_item_tiles((uint32_t)w) * kClusterTriangleTileWords >= cluster_survive_words((uint32_t)w), "W %llu: the tiles hold the words", w);
        }
        CHECK(p.scratch_bytes() >= 12ull * bound && p.scratch_bytes() <= 12ull * bound + bound / 8ull + 32ull, "bound %llu: %llu bytes of scratch", bound, p.scratch_bytes());
      }
  std::printf("CLUSTER TRIANGLE PLAN OK %llu\n", checks);
  return 0;
}
