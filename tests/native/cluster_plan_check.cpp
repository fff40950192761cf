// cluster_plan_check.cpp — enumerates cluster_plan.hpp (renderer_amd/csrc) over its decision edges: how a level is cut into
// clusters (index counts around every multiple of 3 and of 192), the index count of every run of a level, the bound on a
// call's work items and whether a call runs, the grids and scratch of plan_cluster_cull around every tile edge and the
// block cap, and the diagnostic build's tile permutations (a bijection for every tile count). Plain C++, no HIP: built by
// tests/test_cluster_restatement.py with g++ -fsanitize=address,undefined. Prints "CLUSTER PLAN OK <checks>". With the argument
// `sizes` it prints the plan's tile sizes and block cap as one JSON line instead: the GPU tests read their edges from it.
#include "../../renderer_amd/csrc/cluster_plan.hpp"

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
    std::printf("{\"instance_tile\": %u, \"item_tile\": %u, \"head_tile\": %u, \"max_blocks\": %u}\n", kClusterInstanceTile, kClusterItemTile, kClusterHeadTile,
                kClusterMaxBlocks);
    return 0;
  }
  static_assert(kClusterTriangles == 64 && kClusterIndices == 192, "the header's constant");
  static_assert(cluster_level_clusters(192) == 1 && cluster_level_clusters(195) == 2, "usable at compile time");
  static_assert(plan_cluster_cull(1, 1).cull_blocks == 1, "usable at compile time");

  // levels: T = floor(len / 3), C = ceil(T / 64), the clusters tile the triangles, the last one may be short
  for (uint32_t len = 0; len <= 192u * 70u + 5u; ++len) {
    const uint32_t t = cluster_level_triangles(len), c = cluster_level_clusters(len);
    CHECK(t == len / 3u && 3u * t <= len && len - 3u * t < 3u, "len %u: T %u", len, t);
    CHECK((unsigned long long)c * 64u >= t && (c == 0u || (unsigned long long)(c - 1u) * 64u < t), "len %u: C %u", len, c);
    uint32_t sum = 0;
    for (uint32_t k = 0; k < c; ++k) {
      const uint32_t n = cluster_triangles(k, t);
      CHECK(n >= 1u && n <= 64u && (n == 64u || k + 1u == c), "len %u cluster %u: %u triangles", len, k, n);
      sum += n;
    }
    CHECK(sum == t, "len %u: the clusters hold %u of %u triangles", len, sum, t);
  }
  for (uint32_t len : {0xFFFFFFFFu, 0xFFFFFFFEu, 0xFFFFFFFDu, 0x80000000u})
    CHECK(cluster_level_clusters(len) == (len / 3u + 63u) / 64u && cluster_level_clusters(len) < (1u << 31), "len %u", len);

  // runs: every (c, run) of levels around the cluster edges = the sum of the clusters' triangles, x 3
  for (uint32_t t : {1u, 63u, 64u, 65u, 127u, 128u, 129u, 640u, 641u}) {
    const uint32_t c_total = (t + 63u) / 64u;
    for (uint32_t c = 0; c < c_total; ++c)
      for (uint32_t run = 1; c + run <= c_total; ++run) {
        uint32_t tris = 0;
        for (uint32_t k = c; k < c + run; ++k) tris += cluster_triangles(k, t);
        CHECK(cluster_run_index_count(c, run, t) == 3u * tris, "T %u c %u run %u", t, c, run);
      }
    CHECK(cluster_run_index_count(0, c_total, t) == 3u * t, "the whole level, T %u", t);
  }
  {  // the largest level: no 32-bit product wraps
    const uint32_t t = 0xFFFFFFFFu / 3u, c_total = (t + 63u) / 64u;
    CHECK(cluster_run_index_count(c_total - 1u, 1, t) == 3u * (t - (c_total - 1u) * 64u), "the last cluster of the largest level");
    CHECK(cluster_run_index_count(0, c_total, t) == 3u * t, "the whole largest level");
  }

  // the bound and the decision
  CHECK(cluster_work_bound(1000, 7, 0) == 7000ull, "own bound");
  CHECK(cluster_work_bound(1000, 7, 5) == 5ull, "the caller's bound");
  CHECK(cluster_work_bound(0xFFFFFFFFu, 0xFFFFFFFFu, 0) == kClusterMaxWork, "clamped");
  CHECK(cluster_work_bound(1, 1, 0xFFFFFFFFu) == kClusterMaxWork, "the largest caller's bound");
  CHECK(cluster_work_bound(5, 0, 0) == 0ull, "a table without clusters");
  for (unsigned long long bound : {0ull, 1ull, 1024ull, kClusterMaxWork})
    for (unsigned long long w : {0ull, 1ull, 1023ull, 1024ull, 1025ull, kClusterMaxWork - 1ull, kClusterMaxWork, kClusterMaxWork + 1ull, 1ull << 40})
      CHECK(cluster_work_fits(w, bound) == (w <= bound && w < (1ull << 32)), "W %llu bound %llu", w, bound);

  // tiles of a W read from device memory
  for (uint32_t w : {0u, 1u, 63u, 64u, 65u, 1023u, 1024u, 1025u, 16383u, 16384u, 16385u, 0xFFFFFFFFu}) {
    CHECK((unsigned long long)cluster_item_tiles(w) * kClusterItemTile >= w && (w == 0u ? cluster_item_tiles(w) == 0u : (unsigned long long)(cluster_item_tiles(w) - 1u) * kClusterItemTile < w), "item tiles of %u", w);
    CHECK((unsigned long long)cluster_survive_words(w) * 64u >= w && (w == 0u ? cluster_survive_words(w) == 0u : (unsigned long long)(cluster_survive_words(w) - 1u) * 64u < w), "words of %u", w);
    CHECK((unsigned long long)cluster_head_tiles(w) * kClusterHeadTile >= w && (w == 0u ? cluster_head_tiles(w) == 0u : (unsigned long long)(cluster_head_tiles(w) - 1u) * kClusterHeadTile < w), "head tiles of %u", w);
    CHECK((unsigned long long)cluster_head_tiles(w) * kClusterHeadTileWords >= cluster_survive_words(w), "the head tiles cover the words of %u", w);
  }

  // the plan: around every tile edge and the block cap
  const unsigned long long cull_cap = (unsigned long long)kClusterMaxBlocks * kClusterItemTile, head_cap = (unsigned long long)kClusterMaxBlocks * kClusterHeadTile;
  for (uint32_t n : {1u, 1023u, 1024u, 1025u, 2048u, 2049u, 1u << 20, 0xFFFFFFFFu})
    for (unsigned long long bound : {0ull, 1ull, 63ull, 64ull, 65ull, 1023ull, 1024ull, 1025ull, 16383ull, 16384ull, 16385ull, cull_cap - 1, cull_cap, cull_cap + 1,
                                     head_cap - 1, head_cap, head_cap + 1, kClusterMaxWork}) {
      const ClusterPlan p = plan_cluster_cull(n, bound);
      CHECK(p.instance_tiles >= 1u && (unsigned long long)p.instance_tiles * kClusterInstanceTile >= n && (unsigned long long)(p.instance_tiles - 1u) * kClusterInstanceTile < n,
            "n %u: %u instance tiles", n, p.instance_tiles);
      const unsigned long long item_tiles = (bound + kClusterItemTile - 1) / kClusterItemTile, head_tiles = (bound + kClusterHeadTile - 1) / kClusterHeadTile;
      CHECK(p.cull_blocks >= 1u && p.cull_blocks <= kClusterMaxBlocks && (item_tiles <= kClusterMaxBlocks ? p.cull_blocks == (item_tiles ? item_tiles : 1ull) : p.cull_loops()),
            "bound %llu: %u cull blocks", bound, p.cull_blocks);
      CHECK(p.head_blocks >= 1u && p.head_blocks <= kClusterMaxBlocks && (head_tiles <= kClusterMaxBlocks ? p.head_blocks == (head_tiles ? head_tiles : 1ull) : p.head_blocks == kClusterMaxBlocks),
            "bound %llu: %u head blocks", bound, p.head_blocks);
      CHECK(p.survive_words * 64ull >= bound && (bound == 0ull || (p.survive_words - 1ull) * 64ull < bound), "bound %llu: %llu words", bound, p.survive_words);
      CHECK(p.head_tiles >= 1u && p.head_tiles >= head_tiles && (unsigned long long)p.head_tiles * kClusterHeadTileWords >= p.survive_words, "bound %llu: %u head tiles", bound, p.head_tiles);
      // whatever W the device finds under the bound, its tiles have rows and words
      if (bound <= kClusterMaxWork) {
        CHECK(cluster_head_tiles((uint32_t)bound) <= p.head_tiles && cluster_survive_words((uint32_t)bound) <= p.survive_words, "bound %llu: rows for every W", bound);
      }
    }

  // the permutations: bijections of [0, n_tiles)
  for (uint32_t order : {kClusterOrderNone, kClusterOrderReverse, kClusterOrderScramble})
    for (uint32_t tiles : {1u, 2u, 3u, 16u, 17u, 7919u, 7919u * 2u, 104729u}) {
      std::vector<unsigned char> seen(tiles, 0);
      for (uint32_t t = 0; t < tiles; ++t) {
        const uint32_t to = cluster_permute_tile(t, tiles, order);
        CHECK(to < tiles && !seen[to], "order %u, %u tiles: tile %u -> %u", order, tiles, t, to);
        seen[to] = 1;
      }
      if (order == kClusterOrderReverse) CHECK(cluster_permute_tile(0, tiles, order) == tiles - 1u, "reversed");
      if (order == kClusterOrderNone) CHECK(cluster_permute_tile(tiles - 1u, tiles, order) == tiles - 1u, "identity");
    }
  std::printf("CLUSTER PLAN OK %llu\n", checks);
  return 0;
}
