// cluster_phase_plan_check.cpp — enumerates what cluster_plan.hpp (renderer_amd/csrc) adds for mip_cull_clusters_phase over
// its decision edges: the size of a record around every multiple of 64 work items and at the largest W, the work items a
// record of a given size has words for (the inverse: a record of cluster_record_bytes(w) holds w and one byte less does not),
// and the retest kernel's grid, which walks the item tiles the cull kernel walks. Plain C++, no HIP: built by
// tests/test_cluster_phase_restatement.py with g++ -fsanitize=address,undefined. Prints "CLUSTER PHASE PLAN OK <checks>".
#include "../../renderer_amd/csrc/cluster_plan.hpp"

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

int main() {
  static_assert(cluster_record_bytes(0) == 16 && cluster_record_bytes(1) == 24 && cluster_record_bytes(64) == 24 && cluster_record_bytes(65) == 32,
                "usable at compile time");
  static_assert(cluster_record_bytes(0xFFFFFFFFull) == 16ull + 8ull * (1ull << 26), "the largest W of a call that runs");
  static_assert(cluster_record_items(16) == 0 && cluster_record_items(23) == 0 && cluster_record_items(24) == 64, "usable at compile time");

  // the size: a header and a word per 64 items, begun ones included; it agrees with the survive words of the same W
  for (unsigned long long w = 0; w <= 64ull * 300ull + 5ull; ++w) {
    const unsigned long long bytes = cluster_record_bytes(w), words = (bytes - kClusterRecordHeaderBytes) / 8ull;
    CHECK(bytes % 8ull == 0ull && words * 64ull >= w && (w == 0ull || (words - 1ull) * 64ull < w), "W %llu: %llu bytes", w, bytes);
    CHECK(words == cluster_survive_words((uint32_t)w), "W %llu: %llu record words, %u survive words", w, words, cluster_survive_words((uint32_t)w));
    // the inverse: exactly enough room holds W; a byte less does not (W > 0 in a begun word)
    CHECK(cluster_record_items(bytes) >= w, "W %llu fits its own record", w);
    if (w > 0ull) CHECK(cluster_record_items(bytes - 1ull) < w, "W %llu does not fit a record one byte short", w);
    if (w > 0ull) CHECK(cluster_record_items(bytes - 8ull) < w, "W %llu does not fit a record one word short", w);
  }
  for (unsigned long long w : {0xFFFFFFFFull - 64ull, 0xFFFFFFFFull - 63ull, 0xFFFFFFFFull - 1ull, 0xFFFFFFFFull, 1ull << 32, (1ull << 32) + 1ull, ~0ull - 63ull, ~0ull}) {
    const unsigned long long bytes = cluster_record_bytes(w);
    CHECK(bytes == 16ull + 8ull * (w / 64ull + (w % 64ull ? 1ull : 0ull)), "W %llu: %llu bytes", w, bytes);  // (no 64-bit sum wraps)
  }
  // the room: never more than a call can run, monotone, any size from 16 bytes on
  unsigned long long before = 0;
  for (unsigned long long bytes = 16; bytes <= 16ull + 8ull * 70ull; ++bytes) {
    const unsigned long long items = cluster_record_items(bytes);
    CHECK(items == 64ull * ((bytes - 16ull) / 8ull) && items >= before, "%llu bytes: %llu items", bytes, items);
    before = items;
  }
  for (unsigned long long bytes : {cluster_record_bytes(kClusterMaxWork) - 8ull, cluster_record_bytes(kClusterMaxWork), cluster_record_bytes(kClusterMaxWork) + 8ull, 1ull << 40, ~0ull}) {
    const unsigned long long items = cluster_record_items(bytes);
    CHECK(items <= kClusterMaxWork && (bytes < cluster_record_bytes(kClusterMaxWork) ? items == kClusterMaxWork - 63ull : items == kClusterMaxWork), "%llu bytes: %llu items", bytes, items);
  }
  // a phase call's bound is the smaller of the call's and the record's: the words the kernels touch are inside the record
  for (unsigned long long bound : {0ull, 1ull, 63ull, 64ull, 65ull, 1023ull, 1024ull, 1025ull, 16383ull, 16384ull, 16385ull, kClusterMaxWork})
    for (unsigned long long bytes : {16ull, 24ull, 32ull, 16ull + 8ull * 16ull, 16ull + 8ull * 257ull, cluster_record_bytes(kClusterMaxWork)}) {
      const unsigned long long room = cluster_record_items(bytes), held = room < bound ? room : bound;
      CHECK(cluster_record_bytes(held) <= bytes, "bound %llu, %llu bytes: the record of the bound needs %llu", bound, bytes, cluster_record_bytes(held));
      for (unsigned long long w : {0ull, 1ull, held / 2ull, held})
        if (cluster_work_fits(w, held)) CHECK(16ull + 8ull * cluster_survive_words((uint32_t)w) <= bytes, "W %llu under bound %llu", w, held);
      // the retest grid: the cull kernel's, for every N
      for (uint32_t n : {1u, 1024u, 1025u, 1u << 20}) {
        const ClusterPlan p = plan_cluster_cull(n, held);
        const unsigned long long item_tiles = (held + kClusterItemTile - 1) / kClusterItemTile;
        CHECK(p.retest_blocks == p.cull_blocks && p.retest_blocks >= 1u && p.retest_blocks <= kClusterMaxBlocks, "bound %llu: %u retest blocks", held, p.retest_blocks);
        CHECK(item_tiles <= kClusterMaxBlocks ? p.retest_blocks == (item_tiles ? item_tiles : 1ull) : p.retest_blocks == kClusterMaxBlocks, "bound %llu: %u retest blocks for %llu tiles", held, p.retest_blocks, item_tiles);
      }
    }
  std::printf("CLUSTER PHASE PLAN OK %llu\n", checks);
  return 0;
}
