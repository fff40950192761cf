// batch_merge_kernel.hpp — batched draws for sharded scenes (extension, not reference behaviour): the chunk a shard emits and the
// merge of the all-gathered chunks into the bytes mip_batch_draws_lods writes for the unsharded scene (gfx950).
//
//   chunk = { members, n_buckets, 0, 0 | bucket_count[B] | pad to 16 B | ids[capacity] }        (include/mi_instance_pipeline.h)
//
// PRODUCER (mip_batch_draws_shard): the batched-draws stage itself (batch_kernel.hpp under BatchLodChainKey) with the ids going
// to the chunk; its epilogue, mip_batch_shard_chunk_kernel, takes the command writer's place: bucket totals out densely, the
// header, the pad, and the member count where the list passes read it.
//
// CONSUMER (mip_merge_batches): shards are contiguous draw-index ranges in rank order, so (bucket, rank, slot) order IS
// (bucket, draw index) order. Two launches on one stream; no workgroup waits for another, the order is the kernel boundary.
//
//   offsets  ONE workgroup. Step 1, a wave per chunk and no barrier: the header, the exclusive prefix of the chunk's counts over
//            the buckets (src_start: four counts per lane as one 16-byte load, a DPP scan, a carry) and their exact 64-bit sum
//            -> the chunk is corrupt / overflows / is good. One barrier; a bad chunk ends the call here: two zeros, the status,
//            the error bit, nothing else. Step 2, a thread per bucket: the column sum (coalesced over the buckets), a workgroup
//            scan for first[b], one for the command's entry, one for the segment's entry; the thread writes its bucket's
//            command and its NON-EMPTY (bucket, rank) segments {first output slot, first source slot, rank}, in order.
//   gather   a workgroup per kBatchMergeGatherTile OUTPUT slots, whatever the segments look like: one bucket holding
//            everything and thousands of one-id segments are the same work. The tile finds its first and last segment by
//            binary search in seg_dst (strictly ascending: empty segments are not in the table, so a tile of T slots meets
//            at most T of them), stages them in LDS, and every slot finds its own by binary search there. 4-byte loads and
//            stores, coalesced within a segment: instance_ids may be 4-byte aligned and a segment starts anywhere.
//
// Every address the gather forms comes from counts the offsets kernel has validated: Σ c[r][.] == members[r] <= capacity, so a
// source slot is below the capacity and a destination slot below n_chunks x capacity. The offsets kernel itself reads the
// header, the B counts and the pad of every chunk, all inside MIP_BATCH_CHUNK_IDS_OFFSET(B), whatever the words say.
// Instantiated in api_batch.hip only.
#pragma once

#include "batch_lods_kernel.hpp"
#include "batch_merge_plan.hpp"

namespace mip {

static_assert(kBatchMergeThreads == kTile && kBatchMergeBucketTile == kTile, "batch_block_scan scans one value per thread of a 256-thread workgroup");
static_assert(kMaxBatchChunks == 64, "a chunk per lane where the offsets kernel looks at all of them");

// The most derived argument block of batch_draws() (api_batch.hip): the stage's kernels take their own leading part.
struct ShardBatchArgs : OrderedBatchArgs {
  uint32_t* chunk;  // mip_batch_draws_shard: the chunk's first word; instance_ids points at its ids
};

// ---- the producer's epilogue: one workgroup. bucket_totals == null: no resident instances, every count is 0 ----
static __global__ __launch_bounds__(kTile) __attribute__((unused)) void mip_batch_shard_chunk_kernel(const ShardBatchArgs a) {
  __shared__ uint32_t s_members;
  if (threadIdx.x == 0) s_members = 0u;
  __syncthreads();
  uint32_t* counts = a.chunk + kBatchChunkHeaderWords;
  const uint32_t padded = (uint32_t)batch_chunk_ids_offset_words(a.n_buckets) - kBatchChunkHeaderWords;  // B and the pad words
  uint32_t mine = 0;
  for (uint32_t b = threadIdx.x; b < padded; b += kTile) {
    const uint32_t c = (b < a.n_buckets && a.bucket_totals) ? a.bucket_totals[b] : 0u;
    counts[b] = c;
    mine += c;
  }
  mine = wave_sum(mine);
  if ((threadIdx.x & 63u) == 0u) atomicAdd(&s_members, mine);
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t members = s_members;
    a.chunk[0] = members;
    a.chunk[1] = a.n_buckets;
    a.chunk[2] = 0u;
    a.chunk[3] = 0u;
    if (a.members_out) *a.members_out = members;
  }
}

struct BatchMergeArgs {
  const unsigned char* chunks;
  unsigned long long stride;     // bytes, a multiple of 16
  uint32_t n_chunks;             // R <= 64
  uint32_t n_buckets;            // B of this context's table
  uint32_t capacity;             // ids a chunk may carry
  uint32_t ids_offset_words;     // MIP_BATCH_CHUNK_IDS_OFFSET(B) / 4
  // the table
  const MeshChain* chain;
  const uint32_t* bucket_lod;
  const MeshDraw* mesh_draw;
  // scratch (batch_merge_plan.hpp)
  uint32_t* head;
  uint32_t* src_start;
  uint32_t* seg_dst;
  uint32_t* seg_src;
  uint32_t* seg_rank;
  // outputs
  uint32_t* batch_cmds;
  uint32_t* batch_count;
  uint32_t* instance_count;      // or null
  uint32_t* instance_ids;
  uint32_t* error_flag;          // host-mapped
};

__device__ __forceinline__ const uint32_t* batch_chunk_words(const BatchMergeArgs& a, uint32_t r) {
  return reinterpret_cast<const uint32_t*>(a.chunks + (size_t)r * a.stride);
}

// ---- offsets: validate, reduce the columns, scan the buckets, write commands, counts, status and the segment table ----
static __global__ __launch_bounds__(kTile) __attribute__((unused)) void mip_batch_merge_offsets_kernel(const BatchMergeArgs a) {
  __shared__ uint32_t s_wave[kWaves];
  __shared__ uint32_t s_bad[2];  // [0] corrupt chunks, [1] overflowing chunks
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t B = a.n_buckets, R = a.n_chunks;
  if (tid < 2u) s_bad[tid] = 0u;
  __syncthreads();

  // step 1: chunk r by wave r % 4
  for (uint32_t r = wave; r < R; r += kWaves) {
    const uint32_t* w = batch_chunk_words(a, r);
    const uint4 h = *reinterpret_cast<const uint4*>(w);
    uint32_t carry = 0;
    unsigned long long sum = 0;
    for (uint32_t first = 0; first < B; first += 256u) {
      const uint32_t b0 = first + 4u * lane;
      uint4 c = make_uint4(0u, 0u, 0u, 0u);
      if (b0 < B) c = *reinterpret_cast<const uint4*>(w + kBatchChunkHeaderWords + b0);  // counts and pad: inside the chunk
      if (b0 + 1u >= B) c.y = 0u;
      if (b0 + 2u >= B) c.z = 0u;
      if (b0 + 3u >= B) c.w = 0u;
      sum += (unsigned long long)c.x + c.y + c.z + c.w;
      const uint32_t four = c.x + c.y + c.z + c.w;
      const uint32_t incl = wave_inclusive_scan(four);
      uint32_t at = carry + incl - four;
      uint32_t* dst = a.src_start + (size_t)r * B + b0;
      if (b0 < B) dst[0] = at;
      at += c.x;
      if (b0 + 1u < B) dst[1] = at;
      at += c.y;
      if (b0 + 2u < B) dst[2] = at;
      at += c.z;
      if (b0 + 3u < B) dst[3] = at;
      carry += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
#pragma unroll
    for (uint32_t d = 32u; d >= 1u; d >>= 1) sum += __shfl_xor(sum, (int)d);
    if (lane == 0u) {
      if (h.y != B || h.z != 0u || h.w != 0u || sum != (unsigned long long)h.x) atomicAdd(&s_bad[0], 1u);
      else if (h.x > a.capacity) atomicAdd(&s_bad[1], 1u);
    }
  }
  __syncthreads();  // (also: src_start is visible to the whole workgroup)
  const uint32_t corrupt = s_bad[0], overflow = s_bad[1];
  if (corrupt || overflow) {
    if (tid == 0u) {
      *a.batch_count = 0u;
      if (a.instance_count) *a.instance_count = 0u;
      a.head[0] = 1u;
      a.head[1] = 0u;
      a.head[2] = 0u;
      raise_error(a.error_flag, corrupt ? kErrBatchChunkCorrupt : kErrBatchChunkOverflow);
    }
    return;
  }

  // step 2: every chunk is good, so every sum below is at most R x capacity < 2^32
  uint32_t cmds_before = 0, members_before = 0, segs_before = 0;
  for (uint32_t first = 0; first < B; first += kTile) {
    const uint32_t b = first + tid;
    uint32_t total = 0, segs = 0;
    if (b < B)
      for (uint32_t r = 0; r < R; ++r) {
        const uint32_t c = batch_chunk_words(a, r)[kBatchChunkHeaderWords + b];
        total += c;
        segs += c ? 1u : 0u;
      }
    uint32_t step_members, step_cmds, step_segs;
    const uint32_t slot = members_before + batch_block_scan(total, s_wave, step_members);
    const uint32_t at = cmds_before + batch_block_scan(total ? 1u : 0u, s_wave, step_cmds);
    uint32_t seg = segs_before + batch_block_scan(segs, s_wave, step_segs);
    if (total) {
      const uint32_t ml = a.bucket_lod[b];  // (BatchChainDraw's fields)
      const uint32_t mesh = ml >> 3, lod = ml & 7u;
      const MeshChain& ch = a.chain[mesh];
      uint32_t* o = a.batch_cmds + (size_t)at * kCmdWords;
      o[0] = ch.index_len[lod];
      o[1] = total;
      o[2] = ch.index_offset[lod];
      o[3] = (uint32_t)a.mesh_draw[mesh].vertex_offset;
      o[4] = slot;
      uint32_t to = slot;
      for (uint32_t r = 0; r < R; ++r) {
        const uint32_t c = batch_chunk_words(a, r)[kBatchChunkHeaderWords + b];
        if (c) {
          a.seg_dst[seg] = to;
          a.seg_src[seg] = a.src_start[(size_t)r * B + b];
          a.seg_rank[seg] = r;
          ++seg;
          to += c;
        }
      }
    }
    cmds_before += step_cmds;
    members_before += step_members;
    segs_before += step_segs;
  }
  if (tid == 0u) {
    a.seg_dst[segs_before] = members_before;
    *a.batch_count = cmds_before;
    if (a.instance_count) *a.instance_count = members_before;
    a.head[0] = 0u;
    a.head[1] = segs_before;
    a.head[2] = members_before;
  }
}

// ---- gather: kBatchMergeGatherTile output slots per workgroup ----
static __global__ __launch_bounds__(kTile) __attribute__((unused)) void mip_batch_merge_gather_kernel(const BatchMergeArgs a) {
  constexpr uint32_t T = kBatchMergeGatherTile;
  __shared__ uint32_t s_dst[T + 1], s_src[T], s_rank[T];
  if (a.head[0] != 0u) return;  // a bad chunk: nothing is copied
  const uint32_t segments = a.head[1], members = a.head[2];
  const unsigned long long t0_wide = (unsigned long long)blockIdx.x * T;
  if (t0_wide >= members) return;
  const uint32_t t0 = (uint32_t)t0_wide;
  const uint32_t t1 = members - t0 < T ? members : t0 + T;  // the tile is slots [t0, t1)
  // the last segment that starts at or in front of t0, and of t1 - 1: seg_dst[0] = 0 and the values ascend strictly
  uint32_t lo0 = 0, hi0 = segments, lo1 = 0, hi1 = segments;  // answer in [lo, hi)
  while (hi0 - lo0 > 1u || hi1 - lo1 > 1u) {
    const uint32_t m0 = lo0 + ((hi0 - lo0) >> 1), m1 = lo1 + ((hi1 - lo1) >> 1);
    const uint32_t v0 = a.seg_dst[m0], v1 = a.seg_dst[m1];  // m < segments: inside the table (m == lo once a range is down to one)
    if (hi0 - lo0 > 1u) { if (v0 <= t0) lo0 = m0; else hi0 = m0; }
    if (hi1 - lo1 > 1u) { if (v1 <= t1 - 1u) lo1 = m1; else hi1 = m1; }
  }
  const uint32_t j0 = lo0, n_seg = lo1 - lo0 + 1u;  // <= T: every segment but the first starts at a slot of its own inside the tile
  for (uint32_t i = threadIdx.x; i < n_seg; i += kTile) {
    s_dst[i] = a.seg_dst[j0 + i];
    s_src[i] = a.seg_src[j0 + i];
    s_rank[i] = a.seg_rank[j0 + i];
  }
  __syncthreads();
#pragma unroll
  for (uint32_t k = 0; k < kBatchMergeSlotsPerThread; ++k) {
    const uint32_t s = t0 + k * kTile + threadIdx.x;
    if (s < t1) {
      uint32_t lo = 0, hi = n_seg;
      while (hi - lo > 1u) {
        const uint32_t m = lo + ((hi - lo) >> 1);
        if (s_dst[m] <= s) lo = m; else hi = m;
      }
      const uint32_t* ids = batch_chunk_words(a, s_rank[lo]) + a.ids_offset_words;
      a.instance_ids[s] = ids[s_src[lo] + (s - s_dst[lo])];
    }
  }
}

}  // namespace mip
