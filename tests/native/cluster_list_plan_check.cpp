// cluster_list_plan_check.cpp — renderer_amd/csrc/cluster_list_plan.hpp enumerated on the CPU over its decision edges: the
// list tiles and the grids of every bound around each edge, the index count of every cluster of levels around the cluster
// size, a member's word range and word_member against a scalar loop over member lists whose first items sit on, one before
// and one behind the word edges. Built by tests/test_cluster_list_restatement.py with the host sanitizers. With the argument
// `sizes` it prints the plan's tile sizes and block cap as one JSON line instead: the GPU tests read their edges from it.
#include "../../renderer_amd/csrc/cluster_list_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace mip;

static unsigned long long checks = 0;
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

// word_member's definition, as a scalar loop: the member m with first[m] <= 64 k < first[m + 1]
static uint32_t slow_word_member(const std::vector<uint32_t>& first, uint32_t k) {
  for (uint32_t m = 0; m + 1 < first.size(); ++m)
    if (first[m] <= 64ull * k && 64ull * k < first[m + 1]) return m;
  return 0xffffffffu;
}

static void check_members(const std::vector<uint32_t>& sizes) {
  std::vector<uint32_t> first(1, 0u);  // member_first, and W behind it
  for (uint32_t c : sizes) first.push_back(first.back() + c);
  const uint32_t members = (uint32_t)sizes.size(), w = first.back();
  std::vector<uint32_t> by_member(cluster_survive_words(w), 0xffffffffu);
  for (uint32_t m = 0; m < members; ++m) {
    const ClusterListWordRange r = cluster_list_member_words(first[m], first[m + 1]);
    CHECK(r.lo <= r.hi && r.hi <= by_member.size(), "member %u: [%u, %u) of %zu words", m, r.lo, r.hi, by_member.size());
    for (uint32_t k = r.lo; k < r.hi; ++k) {
      CHECK(by_member[k] == 0xffffffffu, "word %u in two members' ranges", k);
      by_member[k] = m;
    }
  }
  for (uint32_t k = 0; k < by_member.size(); ++k) {
    const uint32_t want = slow_word_member(first, k);
    CHECK(want != 0xffffffffu, "word %u has no member", k);
    CHECK(cluster_list_word_member(first.data(), members, k) == want, "word %u: %u, the loop says %u", k, cluster_list_word_member(first.data(), members, k), want);
    CHECK(by_member[k] == want, "word %u: the ranges say %u, the loop %u", k, by_member[k], want);
  }
}

int main(int argc, char**) {
  if (argc > 1) {
    std::printf("{\"instance_tile\": %u, \"item_tile\": %u, \"list_tile\": %u, \"max_blocks\": %u}\n", kClusterInstanceTile, kClusterItemTile, kClusterListTile,
                kClusterMaxBlocks);
    return 0;
  }
  static_assert(kClusterListTile == 64u * kClusterListTileWords && kClusterListTile % kClusterItemTile == 0u, "a list tile is whole item tiles");
  static_assert(kClusterListDrawVertices == 3u * kClusterTriangles, "every entry is drawn with a whole cluster's vertices");

  // the tiles of W and the plan of a bound, around every edge
  const unsigned long long caps[2] = {(unsigned long long)kClusterMaxBlocks * kClusterItemTile, (unsigned long long)kClusterMaxBlocks * kClusterListTile};
  std::vector<unsigned long long> edges = {0, 1, 64, kClusterItemTile, kClusterListTile, 2ull * kClusterListTile, caps[0], caps[1], kClusterMaxWork - 1};
  for (unsigned long long e : edges)
    for (long long d = -2; d <= 2; ++d) {
      const long long s = (long long)e + d;
      if (s < 0 || (unsigned long long)s > kClusterMaxWork) continue;
      const unsigned long long bound = (unsigned long long)s;
      const ClusterListPlan p = plan_cluster_list(bound);
      const unsigned long long list_tiles = (bound + kClusterListTile - 1) / kClusterListTile, item_tiles = (bound + kClusterItemTile - 1) / kClusterItemTile;
      CHECK(p.word_blocks >= 1u && p.word_blocks <= kClusterMaxBlocks && p.write_blocks >= 1u && p.write_blocks <= kClusterMaxBlocks, "bound %llu", bound);
      CHECK(p.word_blocks == (list_tiles < 1 ? 1 : list_tiles < kClusterMaxBlocks ? list_tiles : kClusterMaxBlocks), "bound %llu: word grid %u", bound, p.word_blocks);
      CHECK(p.write_blocks == (item_tiles < 1 ? 1 : item_tiles < kClusterMaxBlocks ? item_tiles : kClusterMaxBlocks), "bound %llu: write grid %u", bound, p.write_blocks);
      CHECK(p.write_blocks == plan_cluster_cull(1000u, bound).cull_blocks, "bound %llu: the write kernel walks the cull kernel's tiles", bound);
      CHECK(p.words * 64ull >= bound && (p.words == 0 || (p.words - 1) * 64ull < bound), "bound %llu: %llu words", bound, p.words);
      CHECK(p.list_tiles >= 1u && (unsigned long long)p.list_tiles * kClusterListTile >= bound, "bound %llu: %u tile rows", bound, p.list_tiles);
      // every W within the bound finds its words and tiles inside the scratch
      const uint32_t w = (uint32_t)bound;
      CHECK(cluster_survive_words(w) <= p.words && cluster_list_tiles(w) <= p.list_tiles, "W %u outside the scratch", w);
      CHECK((unsigned long long)cluster_list_tiles(w) * kClusterListTile >= w && (w == 0 || (unsigned long long)(cluster_list_tiles(w) - 1) * kClusterListTile < w), "W %u", w);
      if (w) CHECK((cluster_survive_words(w) - 1u) / kClusterListTileWords == cluster_list_tiles(w) - 1u, "W %u: the last word lies in the last tile", w);
    }

  // index_count: every cluster of levels around the cluster size sums to the level's triangles
  for (uint32_t t = 1; t <= 4u * kClusterTriangles + 1u; ++t) {
    const uint32_t clusters = cluster_level_clusters(3u * t);
    uint32_t sum = 0;
    for (uint32_t c = 0; c < clusters; ++c) {
      const uint32_t n = cluster_list_index_count(c, t);
      CHECK(n >= 3u && n <= kClusterIndices && n % 3u == 0u && (n == kClusterIndices || c + 1u == clusters), "T %u cluster %u: %u", t, c, n);
      CHECK(n == cluster_run_index_count(c, 1u, t), "T %u cluster %u: not the one-cluster run's count", t, c);
      sum += n;
    }
    CHECK(sum == 3u * t, "T %u: %u indices", t, sum);
  }

  // word ranges and word_member: first items at 64 k - 1, 64 k, 64 k + 1, members of C = 1, 63, 64, 65, 129, many small ones
  for (uint32_t lead : {1u, 62u, 63u, 64u, 65u, 127u, 128u, 129u, 16383u, 16384u, 16385u})
    for (uint32_t c : {1u, 2u, 63u, 64u, 65u, 129u, 300u}) {
      check_members({lead, c});
      check_members({lead, c, 1u});
      check_members({lead, 1u, c, 1u, 1u, c});
      check_members({c, lead});
    }
  check_members({1u});
  check_members({64u});
  check_members({65u});
  check_members(std::vector<uint32_t>(200, 1u));    // 64 members per word
  check_members(std::vector<uint32_t>(200, 63u));
  check_members(std::vector<uint32_t>(200, 65u));
  {
    std::vector<uint32_t> mixed;
    for (uint32_t k = 0; k < 400; ++k) mixed.push_back(1u + (k * 37u) % 131u);
    check_members(mixed);
  }
  std::printf("CLUSTER LIST PLAN OK %llu\n", checks);
  return 0;
}
