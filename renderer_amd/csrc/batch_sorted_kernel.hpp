// batch_sorted_kernel.hpp — globally depth-sorted batched draws (mip_batch_draws_sorted; extension, not reference behaviour):
// the key policy that sorts the members by depth ACROSS buckets, the sum that gives the list its length, and the run stage
// that merges neighbouring slots of one bucket into one instanced command. The sort itself is batch_kernel.hpp's stage.
//
//   U   = 0x7F800000 if q is NaN, else bits(q)                      MIP_DEPTH_RADIAL: the q of the selection rule
//   z   = (e.x*axis.x + e.y*axis.y) + e.z*axis.z, e = pos - cam     MIP_DEPTH_VIEW_AXIS
//   U   = 0xFF800000 if z is NaN, else flip(z == 0 ? 0 : bits(z))   flip(u) = u ^ 0x80000000 (sign clear), ~u (sign set)
//   K   = U >> (32 - depth_bits)
//   D   = K (near first)  or  (Umax >> (32 - depth_bits)) - K (far first)        Umax = 0x7F800000 / 0xFF800000
//
// in float32, contraction off (include/mi_instance_pipeline.h states the rule; tests/sorted_restatement.py restates it).
// The key is D ALONE: depth_bits / 8 passes, pass 0 under BatchSortedKey from the instance columns, the others the list
// kernels of batch_kernel.hpp. No D is kBatchNone: U <= 0xFF800000. The bucket is not in the key, so pass 0's count also
// stores every member's bucket by instance (bucket_out, 4 B per instance, coalesced) and the run stage gathers it through
// instance_ids. No bucket histogram and no bucket command writer: mip_batch_sorted_members_kernel sums pass 0's 256 digit
// totals into the list's length and instance_count, in the place the command writer has after pass 0's rowscan.
//
// The run stage, after the last scatter (slot s is a HEAD if s == 0 or its bucket differs from slot s - 1's):
//
//   run_heads     one 1 024-slot tile per workgroup: b(s) = bucket_out[instance_ids[s] - base] -> slot_bucket[s]; the tile's
//                 number of heads -> counts[tile]. A round's first lane gathers b(s - 1) itself, so no lane reads what
//                 another workgroup (or wave) writes in this launch.
//   rowscan       mip_batch_rowscan_kernel on that one row: exclusive prefixes in place, the sum -> batch_count
//   run_commands  one tile per workgroup: head flags again from slot_bucket (coalesced), a head's rank inside the tile by
//                 ballots, + counts[tile] = its command; words 0, 2, 3 (BatchChainDraw) and 4 (the head's slot)
//   run_counts    one command per lane, batch_count read from device memory under a grid sized for N:
//                 instanceCount[r] = firstInstance[r + 1] - firstInstance[r], `members` for the last command
//
// Closing every run in a launch of its own costs 12 B per COMMAND and spares a segmented scan inside the tile plus the case of
// a run that leaves it. No workgroup waits for another; nothing depends on the order workgroups start in (the diagnostic
// build permutes the tiles of all three kernels). Instantiated in api_batch.hip only.
#pragma once

#include "batch_lods_kernel.hpp"

#pragma clang fp contract(off)

namespace mip {

constexpr uint32_t kDepthRadial = MIP_DEPTH_RADIAL, kDepthViewAxis = MIP_DEPTH_VIEW_AXIS;
constexpr uint32_t kSortedUmaxRadial = 0x7F800000u;  // bits(+inf): the largest U of a q, and the U of a NaN
constexpr uint32_t kSortedUmaxAxis = 0xFF800000u;    // flip(bits(+inf)): the largest U of a z, and the U of a NaN
static_assert(kSortedUmaxAxis < kBatchNone && kSortedUmaxRadial < kBatchNone, "no key is kBatchNone, at any depth_bits");

struct SortedBatchArgs : LodBatchArgs {
  uint32_t depth_shift;     // 32 - depth_bits
  uint32_t depth_flip;      // 0: D = K (near first); Umax >> depth_shift (never 0): D = that - K (far first)
  float axis[3];            // MIP_DEPTH_VIEW_AXIS
  uint32_t* bucket_out;     // pass 0's count: the bucket of every member, by instance; null in every other launch
  // the run stage
  const uint32_t* bucket_in;  // what bucket_out wrote
  uint32_t* slot_bucket;      // the bucket of every slot (a list buffer the sort no longer needs)
};

// U of the squared distance q the selection rule forms: q >= 0 or NaN, so its bit pattern is monotone in its value.
__device__ __forceinline__ uint32_t sorted_u_radial(float q) { return q != q ? kSortedUmaxRadial : __float_as_uint(q); }

// U of a signed distance z: monotone in z, both zeros equal, a NaN as +inf.
__device__ __forceinline__ uint32_t sorted_u_axis(float z) {
  const uint32_t u = z == 0.0f ? 0u : __float_as_uint(z);
  const uint32_t flipped = (u & 0x80000000u) ? ~u : u ^ 0x80000000u;
  return z != z ? kSortedUmaxAxis : flipped;
}

// D of instance il under the policy, the metric and the order, or kBatchNone when it is not a member: lod_chain_pick forms q
// once, for the LOD count and (RADIAL) the key. VIEW_AXIS reads the position lod_chain_pick already loaded.
template <uint32_t kMode, uint32_t kMetric>
struct BatchSortedKey : BatchInstanceKey<BatchSortedKey<kMode, kMetric>, SortedBatchArgs> {
  static constexpr BatchBucketHist kBucketHist = BatchBucketHist::never;  // the run stage counts; nothing is binned by bucket
  static __device__ __forceinline__ uint32_t key(const SortedBatchArgs& a, uint32_t il, bool active) {
    const LodChainPick s = lod_chain_pick<kMode>(a, il, active);
    uint32_t u;
    if constexpr (kMetric == kDepthViewAxis) {
      const float ex = a.pos[3 * (size_t)il + 0] - a.cam[0], ey = a.pos[3 * (size_t)il + 1] - a.cam[1], ez = a.pos[3 * (size_t)il + 2] - a.cam[2];
      const float z = (ex * a.axis[0] + ey * a.axis[1]) + ez * a.axis[2];
      u = sorted_u_axis(z);
    } else {
      u = sorted_u_radial(s.q);
    }
    const uint32_t k = u >> a.depth_shift;
    const uint32_t depth = a.depth_flip ? a.depth_flip - k : k;  // a select, no branch
    if (a.bucket_out && s.member) a.bucket_out[il] = s.bucket;   // il < n: the host sizes it for the context's capacity
    return s.member ? depth : kBatchNone;
  }
  static __device__ __forceinline__ uint32_t bucket_of(uint32_t) { return 0u; }  // (never asked: kBucketHist is never)
};

// ---- the list's length: pass 0's 256 digit totals -> members (the list passes read it) and instance_count. One workgroup. ----
static __global__ __launch_bounds__(kTile) __attribute__((unused)) void mip_batch_sorted_members_kernel(const BatchArgs a) {
  __shared__ uint32_t s_wave[kWaves];
  uint32_t members;
  (void)batch_block_scan(a.totals[threadIdx.x], s_wave, members);
  if (threadIdx.x == 0) {
    if (a.instance_count) *a.instance_count = members;
    *a.members_out = members;
  }
}

// b(s) of a slot below `members`: the bucket pass 0 stored for the instance behind it (uint32 arithmetic: the base may wrap).
__device__ __forceinline__ uint32_t sorted_slot_bucket(const SortedBatchArgs& a, uint32_t s) {
  return a.bucket_in[a.instance_ids[s] - a.first_instance_base];  // a member's instance: < n
}

// ---- run stage 1: the bucket of every slot, the tile's number of heads ----
static __global__ __launch_bounds__(kTile) __attribute__((unused)) void mip_batch_run_heads_kernel(const SortedBatchArgs a) {
  __shared__ uint32_t s_wave[kWaves];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t tile = batch_tile(a);
  const uint32_t members = *a.members;
  uint32_t heads = 0;
#pragma unroll
  for (uint32_t r = 0; r < kBatchRounds; ++r) {
    const uint32_t s = batch_index(tile, wave, r, lane);
    const bool valid = s < members;
    const uint32_t b = valid ? sorted_slot_bucket(a, s) : kBatchNone;
    uint32_t before = (uint32_t)__shfl_up((int)b, 1);
    if (lane == 0u) before = (valid && s > 0u) ? sorted_slot_bucket(a, s - 1u) : kBatchNone;  // s - 1 < members
    if (valid) a.slot_bucket[s] = b;
    heads += (uint32_t)__popcll(__ballot(valid && (s == 0u || b != before)));
  }
  if (lane == 0u) s_wave[wave] = heads;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t total = 0;
#pragma unroll
    for (uint32_t w = 0; w < kWaves; ++w) total += s_wave[w];
    a.counts[tile] = total;  // row 0 of counts: tile < n_tiles
  }
}

// ---- run stage 3: every head writes words 0, 2, 3 and 4 of its command ----
static __global__ __launch_bounds__(kTile) __attribute__((unused)) void mip_batch_run_commands_kernel(const SortedBatchArgs a) {
  __shared__ uint32_t s_wave[kWaves];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t tile = batch_tile(a);
  const uint32_t members = *a.members;
  if (tile * kBatchTile >= members) return;  // (the whole workgroup: no barrier is skipped by a part of it)
  uint32_t bucket[kBatchRounds], rank[kBatchRounds];
  bool head[kBatchRounds];
  uint32_t in_wave = 0;
#pragma unroll
  for (uint32_t r = 0; r < kBatchRounds; ++r) {
    const uint32_t s = batch_index(tile, wave, r, lane);
    const bool valid = s < members;
    bucket[r] = valid ? a.slot_bucket[s] : kBatchNone;
    const uint32_t before = (valid && s > 0u) ? a.slot_bucket[s - 1u] : kBatchNone;
    head[r] = valid && (s == 0u || bucket[r] != before);
    const unsigned long long mask = __ballot(head[r]);
    rank[r] = in_wave + lanes_below(mask);
    in_wave += (uint32_t)__popcll(mask);
  }
  if (lane == 0u) s_wave[wave] = in_wave;
  __syncthreads();
  uint32_t first = a.counts[tile];  // the heads of the tiles before this one (rowscan)
#pragma unroll
  for (uint32_t w = 0; w < kWaves; ++w) first += w < wave ? s_wave[w] : 0u;
#pragma unroll
  for (uint32_t r = 0; r < kBatchRounds; ++r) {
    if (head[r]) {
      const BatchDraw d = BatchChainDraw::draw(a, bucket[r]);  // a member's bucket: < n_buckets
      uint32_t* o = a.batch_cmds + (size_t)(first + rank[r]) * kCmdWords;  // < heads <= members <= N commands
      o[0] = d.index_count;
      o[2] = d.first_index;
      o[3] = d.vertex_offset;
      o[4] = batch_index(tile, wave, r, lane);  // firstInstance: the head's slot
    }
  }
}

// ---- run stage 4: instanceCount of command r = the distance from its head to the next one, or to `members` ----
static __global__ __launch_bounds__(kTile) __attribute__((unused)) void mip_batch_run_counts_kernel(const SortedBatchArgs a) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t tile = batch_tile(a);
  const uint32_t count = *a.batch_count, members = *a.members;
#pragma unroll
  for (uint32_t r = 0; r < kBatchRounds; ++r) {
    const uint32_t c = batch_index(tile, wave, r, lane);
    if (c < count) {
      uint32_t* o = a.batch_cmds + (size_t)c * kCmdWords;
      const uint32_t next = c + 1u < count ? o[kCmdWords + 4u] : members;
      o[1] = next - o[4];
    }
  }
}

}  // namespace mip
