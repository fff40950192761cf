// cluster_list_phase_plan_check.cpp — renderer_amd/csrc/cluster_list_phase_plan.hpp enumerated on the CPU over its decision
// edges: the launch list of both phases and its grids for every bound around each tile and cap edge, the scratch — the
// candidates' tile row and the two scalars included — against the tiles any W within the bound needs, and the room and the
// count behind every entry base around every capacity. Built by tests/test_cluster_list_phase_restatement.py with the host
// sanitizers. With the argument `sizes` it prints the plan's tile sizes and block cap as one JSON line instead: the GPU tests
// read their edges from it.
#include "../../renderer_amd/csrc/cluster_list_phase_plan.hpp"

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

int main(int argc, char**) {
  if (argc > 1) {
    std::printf("{\"instance_tile\": %u, \"item_tile\": %u, \"list_tile\": %u, \"max_blocks\": %u}\n", kClusterInstanceTile, kClusterItemTile, kClusterListTile,
                kClusterMaxBlocks);
    return 0;
  }
  static_assert(kClusterListPhaseLaunches == 8u && kClusterListPhaseScWords == 2u && kClusterListPhaseScBase != kClusterListPhaseScRoom, "the plan's shape");
  static_assert(plan_cluster_list_phase(1000u, 100000u, true).launches[4].kernel == ClusterListPhaseKernel::front, "constexpr");

  // the launch list, the grids and the scratch of both phases, around every edge of the bound and of N
  const unsigned long long caps[2] = {(unsigned long long)kClusterMaxBlocks * kClusterItemTile, (unsigned long long)kClusterMaxBlocks * kClusterListTile};
  const std::vector<unsigned long long> edges = {0, 1, 64, kClusterItemTile, kClusterListTile, 2ull * kClusterListTile, caps[0], caps[1], kClusterMaxWork - 1};
  const ClusterListPhaseKernel order[8] = {ClusterListPhaseKernel::count, ClusterListPhaseKernel::scan, ClusterListPhaseKernel::members, ClusterListPhaseKernel::word_members,
                                          ClusterListPhaseKernel::front, ClusterListPhaseKernel::list_count, ClusterListPhaseKernel::list_epilogue, ClusterListPhaseKernel::list_write};
  for (uint32_t n : {1u, 1023u, 1024u, 1025u, 1000000u})
    for (unsigned long long e : edges)
      for (long long d = -2; d <= 2; ++d) {
        const long long s = (long long)e + d;
        if (s < 0 || (unsigned long long)s > kClusterMaxWork) continue;
        const unsigned long long bound = (unsigned long long)s;
        for (bool first : {true, false}) {
          const ClusterListPhasePlan p = plan_cluster_list_phase(n, bound, first);
          const ClusterPlan front = plan_cluster_cull(n, bound);
          const ClusterListPlan list = plan_cluster_list(bound);
          for (uint32_t k = 0; k < kClusterListPhaseLaunches; ++k) {
            CHECK(p.launches[k].kernel == order[k], "bound %llu: launch %u", bound, k);
            CHECK(p.launches[k].blocks >= 1u, "bound %llu: launch %u has no workgroup", bound, k);
          }
          // word_members stands in front of the front: the front reads word_member
          CHECK(p.launches[0].blocks == front.instance_tiles && p.launches[2].blocks == front.instance_tiles, "bound %llu n %u: instance tiles", bound, n);
          CHECK((unsigned long long)p.launches[0].blocks * kClusterInstanceTile >= n, "n %u: %u instance tiles", n, p.launches[0].blocks);
          CHECK(p.launches[1].blocks == 1u && p.launches[6].blocks == 1u, "bound %llu: scan and epilogue are one workgroup", bound);
          CHECK(p.launches[3].blocks == list.word_blocks && p.launches[5].blocks == list.word_blocks, "bound %llu: word grids", bound);
          CHECK(p.launches[4].blocks == (first ? front.cull_blocks : front.retest_blocks), "bound %llu: the front's grid is the phase call's", bound);
          CHECK(p.launches[7].blocks == list.write_blocks && list.write_blocks == front.cull_blocks, "bound %llu: the write kernel walks the front's tiles", bound);
          for (uint32_t k : {3u, 4u, 5u, 7u}) CHECK(p.launches[k].blocks <= kClusterMaxBlocks, "bound %llu: launch %u above the cap", bound, k);
          // scratch: every W within the bound finds its words and both tile rows inside it
          const uint32_t w = (uint32_t)bound;
          CHECK(p.survive_words >= cluster_survive_words(w) && p.member_words >= cluster_survive_words(w) && p.rank_words >= cluster_survive_words(w), "W %u: words", w);
          CHECK(p.tile_rows >= cluster_list_tiles(w) && p.tile_rows >= 1u, "W %u: %u tile rows", w, p.tile_rows);
          CHECK(p.candidate_rows == (first ? p.tile_rows : 0u), "bound %llu: the candidates' row is FIRST's", bound);
          CHECK(p.scalar_words == kClusterListPhaseScWords, "bound %llu: scalars", bound);
          CHECK(p.list_scratch_bytes() == 4ull * (2ull * list.words + (first ? 2ull : 1ull) * list.list_tiles + 2ull), "bound %llu: %llu bytes", bound, p.list_scratch_bytes());
          // a looping grid reaches every tile: tile = block, block + grid, ...
          if (w) {
            CHECK(cluster_item_tiles(w) <= (unsigned long long)p.launches[4].blocks * ((cluster_item_tiles(w) + p.launches[4].blocks - 1u) / p.launches[4].blocks), "W %u", w);
            CHECK((cluster_survive_words(w) - 1u) / kClusterListTileWords == cluster_list_tiles(w) - 1u, "W %u: the last word lies in the last list tile", w);
          }
        }
      }

  // the base: room = capacity - min(b, capacity); count = min(survivors, room); b + count never leaves the buffer
  const std::vector<uint32_t> values = {0u, 1u, 2u, 63u, 64u, 65u, 1000u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
  for (uint32_t capacity : values)
    for (uint32_t b0 : values)
      for (int db = -1; db <= 1; ++db) {
        const uint32_t b = b0 + (uint32_t)db;  // wraps at the ends: every value is a legal base
        const uint32_t room = cluster_list_phase_room(b, capacity);
        CHECK(room <= capacity, "b %u capacity %u: room %u", b, capacity, room);
        CHECK(b >= capacity ? room == 0u : room == capacity - b, "b %u capacity %u: room %u", b, capacity, room);
        for (uint32_t survivors : values) {
          const uint32_t count = cluster_list_phase_count(survivors, b, capacity);
          CHECK(count <= survivors && count <= room && (count == survivors || count == room), "b %u capacity %u survivors %u: count %u", b, capacity, survivors, count);
          CHECK(count == 0u || (unsigned long long)b + count <= capacity, "b %u capacity %u: the list leaves the buffer", b, capacity);
        }
      }
  std::printf("CLUSTER LIST PHASE PLAN OK %llu\n", checks);
  return 0;
}
