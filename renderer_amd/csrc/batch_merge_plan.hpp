// batch_merge_plan.hpp — the shard chunk of batched draws and what mip_merge_batches launches: the chunk layout as
// include/mi_instance_pipeline.h states it, the sizes of the two merge kernels (batch_merge_kernel.hpp), their grid and
// their scratch, and the two error bits the offsets kernel raises. Plain C++, no HIP: enumerated on the CPU by
// tests/native/batch_merge_plan_check.cpp; the GPU tests read the tile sizes from here.
#pragma once

#include <cstdint>

namespace mip {

constexpr uint32_t kMaxBatchChunks = 64;             // MIP_MAX_BATCH_CHUNKS = kMaxMergeChunks (merge_kernel.hpp)
constexpr uint32_t kBatchChunkHeaderWords = 4;       // MipBatchChunkHeader {members, n_buckets, 0, 0}
constexpr uint32_t kBatchMergeThreads = 256;         // threads of either kernel's workgroup
constexpr uint32_t kBatchMergeBucketTile = 256;      // buckets the offsets kernel takes per step: a thread each (a wave's step of the
                                                     // per-rank scan: a lane takes four consecutive counts as one 16-byte load)
constexpr uint32_t kBatchMergeSlotsPerThread = 8;
constexpr uint32_t kBatchMergeGatherTile = kBatchMergeThreads * kBatchMergeSlotsPerThread;  // output slots of a gather workgroup
constexpr unsigned long long kBatchMergeMaxTable = 1ull << 24;  // n_chunks x B above this: MIP_ERR_CAPACITY

// Device -> host error bits of the offsets kernel, in the words instance_kernel.hpp's list leaves free (0 and 4).
constexpr uint32_t kErrBatchChunkCorrupt = 1u;    // word 0: a gathered batch chunk breaks the format (MIP_ERR_DEVICE)
constexpr uint32_t kErrBatchChunkOverflow = 16u;  // word 4: a gathered batch chunk holds more members than the exchanged prefix (MIP_ERR_CAPACITY)

// words in front of a chunk's ids: header, B counts, pad to 16 bytes
constexpr unsigned long long batch_chunk_ids_offset_words(unsigned long long buckets) {
  return kBatchChunkHeaderWords + buckets + (4u - buckets % 4u) % 4u;
}
constexpr unsigned long long batch_chunk_bytes(unsigned long long buckets, unsigned long long capacity) {
  return (batch_chunk_ids_offset_words(buckets) + capacity) * 4u;
}

// Scratch words of a merge of n_chunks x B counts, in this order:
//   head[4]                 {status, segments S, members, 0}
//   src_start[n_chunks][B]  where bucket b's ids start in chunk r: the exclusive prefix of c[r][.]
//   seg_dst[S + 1]          first output slot of every NON-EMPTY (bucket, rank) segment, ascending; [S] = members
//   seg_src[S], seg_rank[S] where the segment's ids start in its chunk, and which chunk
struct BatchMergePlan {
  unsigned long long table;          // n_chunks x B
  unsigned long long scratch_words;
  unsigned long long src_start, seg_dst, seg_src, seg_rank;  // word offsets into the scratch
  uint32_t table_steps;              // steps of kBatchMergeBucketTile buckets the offsets kernel's one workgroup takes
  uint32_t gather_blocks;            // workgroups of the gather: the output slots the chunks can hold, at least one
};

constexpr bool batch_merge_table_fits(unsigned long long n_chunks, unsigned long long buckets) { return n_chunks * buckets <= kBatchMergeMaxTable; }
// the merged list has at most n_chunks x capacity slots and their number is a 32-bit word
constexpr bool batch_merge_slots_fit(unsigned long long n_chunks, unsigned long long capacity) { return n_chunks * capacity < (1ull << 32); }

constexpr BatchMergePlan plan_batch_merge(unsigned long long n_chunks, unsigned long long buckets, unsigned long long capacity) {
  BatchMergePlan p{};
  p.table = n_chunks * buckets;
  p.src_start = 4;
  p.seg_dst = p.src_start + p.table;
  p.seg_src = p.seg_dst + p.table + 1;
  p.seg_rank = p.seg_src + p.table;
  p.scratch_words = p.seg_rank + p.table;
  p.table_steps = (uint32_t)((buckets + kBatchMergeBucketTile - 1) / kBatchMergeBucketTile);
  const unsigned long long slots = n_chunks * capacity;
  const unsigned long long blocks = (slots + kBatchMergeGatherTile - 1) / kBatchMergeGatherTile;
  p.gather_blocks = blocks ? (uint32_t)blocks : 1u;
  return p;
}

}  // namespace mip
