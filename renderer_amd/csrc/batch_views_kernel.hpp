// batch_views_kernel.hpp — batched draws over the whole LOD chain for several views in one call (mip_batch_draws_views;
// extension, not reference behaviour). The stage is batch_kernel.hpp's, the selection rule batch_lods_kernel.hpp's
// lod_chain_pick; this header adds the key policy, the per-view first_instance_base of the last scatter and a command
// writer that packs every view's commands into the view's own range.
//
//   entry  e = i * n_views + v        instance-major: the lanes of a wave that share an instance share its loads, so the
//                                     instance columns come from memory once, not n_views times; for a fixed view e ascends
//                                     with i, so the stable binning keeps draw order inside every (view, bucket)
//   key    = v * B + bucket           bucket = lod_base[mesh] + lod as mip_batch_draws_lods forms it for frames[v] and
//                                     visible_bitmaps[v] (a null bitmap: every resident instance), or kBatchNone
//   view   = key / B                  comes back from the key: the last scatter adds that view's first_instance_base
//
// n_views * B <= 256 global buckets: one pass, straight from the instance columns to instance_ids. More: pass 0 writes a
// (key, instance) list and counts the members of every global bucket (bucket_hist, as mip_batch_draws_lods does above 256
// buckets, but in hist_copies copies that the command writer sums), the later passes are the list kernels; only the last of them knows about views (BatchViewsListKey).
// Entries of a view do not align to a tile, and need not: a tile is 1 024 ENTRIES. Instantiated in api_batch.hip only.
#pragma once

#include "batch_lods_kernel.hpp"

#pragma clang fp contract(off)

namespace mip {

constexpr uint32_t kBatchMaxViews = MIP_MAX_VIEWS;

struct ViewBatchArgs : LodBatchArgs {
  uint32_t n_views;
  uint32_t view_buckets;   // B = sum of n_lods; n_buckets = n_views * B
  uint32_t n_entries;      // n_views * n: what n_tiles covers
  uint32_t cmd_stride;     // commands reserved per view
  uint32_t hist_copies;    // several passes: copies of bucket_hist (a power of two), copy = tile & (hist_copies - 1); else 1
  const uint32_t* view_bitmap[kBatchMaxViews];  // null: every resident instance
  float view_cam[kBatchMaxViews][3];
  uint32_t view_base[kBatchMaxViews];           // first_instance_base of every view
  // command kernel
  uint32_t* batch_counts;      // n_views words
  uint32_t* view_first_slot;   // n_views + 1 words, or null
};

// The last scatter of a views call: the view is the key's, and so is the base (batch_kernel.hpp calls this through the
// most derived argument block).
__device__ __forceinline__ uint32_t batch_first_instance(const ViewBatchArgs& a, uint32_t key) {
  return a.view_base[key / a.view_buckets];
}

// Pass 0 of several counts the members of every global bucket with device-scope adds; with a few hundred buckets and
// millions of members those adds queue up on a handful of cache lines, so concurrent tiles add to
// different copies of the histogram and the command writer sums the copies.
__device__ __forceinline__ uint32_t batch_hist_index(const ViewBatchArgs& a, uint32_t bucket, uint32_t tile) {
  return (tile & (a.hist_copies - 1u)) * a.n_buckets + bucket;  // < hist_copies * n_buckets <= 2^20 or n_buckets: the host's rule
}

// v * B + bucket of entry (instance, view), or kBatchNone when the instance is not a member of that view.
template <uint32_t kMode>
struct BatchViewsKey {
  using Args = ViewBatchArgs;
  static constexpr bool kFromList = false;
  static constexpr BatchBucketHist kBucketHist = BatchBucketHist::when_given;  // pass 0 of several
  static __device__ __forceinline__ uint32_t load(const ViewBatchArgs& a, uint32_t idx, uint32_t) {
    const bool active = idx < a.n_entries;
    const uint32_t e = active ? idx : a.n_entries - 1u;  // an idle lane loads the last entry, in bounds
    const uint32_t il = e / a.n_views, v = e - il * a.n_views;
    const uint32_t* bitmap = a.view_bitmap[v];
    const uint32_t word = bitmap ? bitmap[il >> 5] : 0xffffffffu;
    const LodChainPick s = lod_chain_pick<kMode>(a, il, active, word, a.view_cam[v][0], a.view_cam[v][1], a.view_cam[v][2]);
    return s.member ? v * a.view_buckets + s.bucket : kBatchNone;  // < n_views * B <= 2^31
  }
  static __device__ __forceinline__ uint32_t id(const ViewBatchArgs& a, uint32_t idx) { return idx / a.n_views; }
  static __device__ __forceinline__ uint32_t bucket_of(uint32_t key) { return key; }  // the global bucket v * B + bucket
};

// The last list pass of a views call: BatchListKey over the block that holds the views' bases.
struct BatchViewsListKey : BatchListKey {
  using Args = ViewBatchArgs;
};

// ---- commands: per view, one per non-empty bucket of the view, ascending, packed from v * cmd_stride; the view's count
// and first slot. One workgroup walks the n_views * B global buckets 256 at a time: two scans give every bucket its
// absolute slot and the number of non-empty buckets before it, and the first bucket of a view leaves both in LDS for the
// buckets of its view — in this chunk or a later one. ----
static __global__ __launch_bounds__(kTile) __attribute__((unused)) void mip_batch_view_commands_kernel(const ViewBatchArgs a) {
  __shared__ uint32_t s_wave[kWaves];
  __shared__ uint32_t s_view_cmd[kBatchMaxViews + 1], s_view_slot[kBatchMaxViews + 1];
  uint32_t cmds_before = 0, members_before = 0;
  for (uint32_t first = 0; first < a.n_buckets; first += kTile) {  // (n_buckets <= 2^31: the host refuses more)
    const uint32_t g = first + threadIdx.x;
    const bool in = g < a.n_buckets;
    uint32_t c = 0;
    if (in)
      for (uint32_t k = 0; k < a.hist_copies; ++k) c += a.bucket_totals[(size_t)k * a.n_buckets + g];  // `totals`: one copy
    const uint32_t v = in ? g / a.view_buckets : 0u, b = g - v * a.view_buckets;
    uint32_t chunk_members, chunk_cmds;
    const uint32_t slot = members_before + batch_block_scan(c, s_wave, chunk_members);
    const uint32_t at = cmds_before + batch_block_scan(c ? 1u : 0u, s_wave, chunk_cmds);
    if (in && b == 0u) {
      s_view_cmd[v] = at;
      s_view_slot[v] = slot;
    }
    __syncthreads();
    if (c) {
      const BatchDraw d = BatchChainDraw::draw(a, b);
      uint32_t* o = a.batch_cmds + ((size_t)v * a.cmd_stride + (at - s_view_cmd[v])) * kCmdWords;
      o[0] = d.index_count;    // indexCount
      o[1] = c;                // instanceCount
      o[2] = d.first_index;    // firstIndex
      o[3] = d.vertex_offset;  // vertexOffset
      o[4] = slot;             // firstInstance: the absolute slot in the shared instance_ids
    }
    cmds_before += chunk_cmds;
    members_before += chunk_members;
  }
  if (threadIdx.x == 0) {
    s_view_cmd[a.n_views] = cmds_before;
    s_view_slot[a.n_views] = members_before;
    *a.members_out = members_before;
  }
  __syncthreads();
  if (threadIdx.x < a.n_views) a.batch_counts[threadIdx.x] = s_view_cmd[threadIdx.x + 1u] - s_view_cmd[threadIdx.x];
  if (a.view_first_slot && threadIdx.x <= a.n_views) a.view_first_slot[threadIdx.x] = s_view_slot[threadIdx.x];
}

}  // namespace mip
