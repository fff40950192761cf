// batch_merge_plan_check.cpp — enumerates, on the CPU, what the batched draws of a sharded scene launch:
//   * plan_batch (renderer_amd/csrc/batch_plan.hpp) for BatchEntry::shard, both modes, bucket counts either side of every pass
//     boundary (256, 65 536, 2^24): mip_batch_draws_lods' count / rowscan / scatter instantiations pass for pass, never a model
//     kernel, and the chunk epilogue in the command writer's place;
//   * the chunk layout (batch_merge_plan.hpp) against the header's macros;
//   * plan_batch_merge: the scratch layout without overlaps, the offsets kernel's steps, the gather's grid either side of its
//     tile, and the two capacity rules.
// Plain C++, no HIP: built by tests/test_batch_merge_restatement.py with gcc -fsanitize=address,undefined.
// Prints the tile sizes (the GPU tests read them from here) and "BATCH MERGE PLAN OK <combinations>".
#include "../../include/mi_instance_pipeline.h"
#include "../../renderer_amd/csrc/batch_merge_plan.hpp"
#include "../../renderer_amd/csrc/batch_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <set>

using namespace mip;
using K = BatchKernel;

#define CHECK(cond, ...)                                            \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::printf("FAILED %s:%d %s — ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                                     \
      std::printf("\n");                                            \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

int main() {
  static_assert(plan_batch(BatchEntry::shard, false, 200, false, false).commands == K::commands_shard, "usable at compile time");
  static_assert(sizeof(MipBatchChunkHeader) == kBatchChunkHeaderWords * 4 && MIP_MAX_BATCH_CHUNKS == kMaxBatchChunks, "the header's chunk");
  unsigned long long combos = 0;

  // ---- the producer: the lods plan with the chunk epilogue ----
  std::set<unsigned long long> buckets = {1, 2, 6, 200, 4097};
  for (unsigned long long edge : {256ull, 65536ull, 1ull << 24})
    for (long long d = -1; d <= 2; ++d) buckets.insert(edge + (unsigned long long)d);
  for (unsigned long long b : buckets)
    for (int relative = 0; relative < 2; ++relative)
      for (int want_model = 0; want_model < 2; ++want_model)
        for (int general = 0; general < 2; ++general) {
          ++combos;
          const BatchPlan s = plan_batch(BatchEntry::shard, relative != 0, b, want_model != 0, general != 0);
          const BatchPlan l = plan_batch(BatchEntry::lods, relative != 0, b, false, false);
          CHECK(s.passes == (b <= 256 ? 1u : b <= 65536 ? 2u : b <= (1ull << 24) ? 3u : 4u), "%llu buckets: %u passes", b, s.passes);
          CHECK(s.passes == l.passes && s.several() == (b > 256), "the passes of mip_batch_draws_lods");
          CHECK(s.commands == K::commands_shard && l.commands == K::commands_chain, "the chunk epilogue takes the command writer's place");
          CHECK(s.model == K::none, "a shard stores no matrices, whatever the flags say");
          for (uint32_t p = 0; p < s.passes; ++p) {
            CHECK(s.count(p) == l.count(p), "count, pass %u of %u", p, s.passes);
            CHECK(s.scatter(p) == l.scatter(p), "scatter, pass %u of %u", p, s.passes);
          }
          const K want0 = s.several() ? (relative ? K::scatter_chain_relative_mid : K::scatter_chain_distance_mid)
                                      : (relative ? K::scatter_chain_relative_last : K::scatter_chain_distance_last);
          CHECK(s.scatter0 == want0 && s.count0 == (relative ? K::count_chain_relative : K::count_chain_distance), "pass 0 forms the chain's keys, ids only");
          CHECK(s.scatter(s.passes - 1) == (s.several() ? K::scatter_list_last : want0), "the last pass writes the chunk's ids");
        }
  // the other entry points are what they were
  CHECK(plan_batch(BatchEntry::lods, false, 200, true, false).scatter0 == K::scatter_chain_distance_model, "lods");
  CHECK(plan_batch(BatchEntry::draws, false, 128, false, false).commands == K::commands_pair, "draws");
  CHECK(plan_batch(BatchEntry::views, true, 300, false, false).commands == K::commands_views, "views");

  // ---- the chunk ----
  for (unsigned long long b = 1; b <= 1030; ++b) {
    ++combos;
    const unsigned long long off = batch_chunk_ids_offset_words(b);
    CHECK(off * 4 == MIP_BATCH_CHUNK_IDS_OFFSET(b), "ids offset of %llu buckets", b);
    CHECK(off % 4 == 0 && off >= 4 + b && off < 4 + b + 4, "the ids start at the first multiple of 16 bytes behind the counts");
    for (unsigned long long cap : {0ull, 1ull, 5ull, 4097ull, 0xffffffffull})
      CHECK(batch_chunk_bytes(b, cap) == MIP_BATCH_CHUNK_BYTES(b, cap) && batch_chunk_bytes(b, cap) == (off + cap) * 4, "chunk bytes");
  }
  CHECK(MIP_BATCH_CHUNK_IDS_OFFSET(200) == 16 + 800 && MIP_BATCH_CHUNK_IDS_OFFSET(3) == 32 && MIP_BATCH_CHUNK_BYTES(3, 2) == 40, "worked values");

  // ---- the merge ----
  const unsigned long long T = kBatchMergeGatherTile, S = kBatchMergeBucketTile;
  CHECK(T == (unsigned long long)kBatchMergeThreads * kBatchMergeSlotsPerThread && S == kBatchMergeThreads, "tiles");
  for (unsigned long long r : {1ull, 2ull, 3ull, 8ull, 63ull, 64ull})
    for (unsigned long long b : {1ull, 6ull, 200ull, S - 1, S, S + 1, 2 * S, 2 * S + 1, 4097ull, 262144ull})
      for (unsigned long long cap : {0ull, 1ull, T / r, T / r + 1, T - 1, T, T + 1, 3 * T, 125000ull}) {
        ++combos;
        const BatchMergePlan p = plan_batch_merge(r, b, cap);
        CHECK(p.table == r * b, "table");
        CHECK(p.src_start == 4 && p.seg_dst == p.src_start + p.table && p.seg_src == p.seg_dst + p.table + 1 &&
              p.seg_rank == p.seg_src + p.table && p.scratch_words == p.seg_rank + p.table, "the scratch arrays follow each other");
        CHECK(p.table_steps == (b + S - 1) / S && (unsigned long long)p.table_steps * S >= b, "%llu buckets: %u steps", b, p.table_steps);
        const unsigned long long slots = r * cap;
        CHECK(p.gather_blocks >= 1 && (unsigned long long)p.gather_blocks * T >= slots, "every slot has a workgroup");
        CHECK(p.gather_blocks == 1 || ((unsigned long long)p.gather_blocks - 1) * T < slots, "and no workgroup is without a possible slot");
      }
  CHECK(batch_merge_table_fits(64, 262144) && !batch_merge_table_fits(64, 262145), "64 chunks: 2^24 counts fit, one bucket more does not");
  CHECK(batch_merge_table_fits(1, 1ull << 24) && !batch_merge_table_fits(1, (1ull << 24) + 1), "one chunk");
  CHECK(batch_merge_slots_fit(64, (1ull << 26) - 1) && !batch_merge_slots_fit(64, 1ull << 26), "64 chunks x capacity < 2^32");
  CHECK(batch_merge_slots_fit(1, 0xffffffffull) && batch_merge_slots_fit(3, 0), "one chunk of any capacity");
  CHECK(kErrBatchChunkCorrupt == 1u && kErrBatchChunkOverflow == 16u, "error words 0 and 4");

  std::printf("BUCKET_TILE %u\nGATHER_TILE %u\n", kBatchMergeBucketTile, kBatchMergeGatherTile);
  std::printf("BATCH MERGE PLAN OK %llu\n", combos);
  return 0;
}
