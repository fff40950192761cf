// cluster_views_list_kernel.hpp — mip_list_clusters_views (the visible-cluster lists for several views in one call; extension,
// not reference behaviour), gfx950: mip_cull_clusters_views' front with mip_list_clusters' 16-byte entries behind it, one list
// and one indirect draw per view. include/mi_instance_pipeline.h specifies it, tests/cluster_views_list_restatement.py restates
// it in numpy, cluster_views_list_plan.hpp holds the arithmetic that is not a kernel. Instantiated in api_cluster.hip only.
//
// The front is mip_cull_clusters_views' own first four launches, unchanged: count, scan, members, cull. They leave plane 0
// (start words) and planes 1 + v (view v's survive words) in view_words. Behind them, on the same stream:
//
//   word members  cluster_list_kernel.hpp's kernel, unchanged, ONCE for all views: a work item is common to every view, so
//                 word_member[k], the member of work item 64 k, is too
//   count         grid row = view, as the several-view heads kernel: one survive word of view v per thread, a tile of 256 words
//                 per workgroup: popcount -> word_rank plane v, the tile's total -> list_tiles row v. A row per view and not a
//                 loop over the views inside: the views share nothing here (one word, one popcount), so a loop would only run
//                 n_views block scans one behind the other in a workgroup that a small W leaves alone on the device
//   epilogue      one workgroup per view: row v becomes exclusive prefixes; entry_counts[v], draw_args[4 v ..], survivors_v,
//                 the status; the workgroup of view 0 also writes W and members. Of a call the scan refused (W = 0 here) this
//                 is the refusal: zero counts, {192, 0, 0, v x entry_stride}, {W, members, 0, ...}
//   write         the hot path, the cull kernel's shape: 64 work items per wave and round. Lane v loads view v's survive word
//                 and the view's survivors in front of it (tile prefix + word rank); every word zero: nothing more. Else
//                 word_member, the 64 member_first entries, the six shuffles of cluster_list_locate and first_index /
//                 vertex_offset / index_count ONCE, kept in registers; then a wave-uniform loop over the views: view v's
//                 words out of lane v (readlane), the rank, and ONE 16-byte store per surviving lane below entry_stride, with
//                 view v's base in `instance`
//
// No workgroup waits for another and nothing depends on the order workgroups start in; the looping grids are capped
// (cluster_list_plan.hpp) and the diagnostic build permutes their tiles.
#pragma once

#include "cluster_views_kernel.hpp"
#include "cluster_list_kernel.hpp"
#include "cluster_views_list_plan.hpp"

#pragma clang fp contract(off)

namespace mip {

struct ClusterViewsListArgs {
  ClusterViewArgs v;             // the front's arguments, as its kernels take them (cmds / cmd_count / stats / tile_heads / tile_survivors unused)
  // scratch
  const uint32_t* word_member;   // per 64 work items, common to all views: the member of the word's first item
  uint32_t* word_rank;           // n_views planes of rank_stride: view v's survivors of the word's list tile in front of the word
  uint32_t* list_tiles;          // n_views rows of tile_stride: survivors, then (epilogue) the survivors of the tiles before
  unsigned long long rank_stride;
  uint32_t tile_stride;
  // outputs
  uint4* entries;                // MipClusterEntry: view v's from v x entry_stride
  uint32_t entry_stride;
  uint32_t* entry_counts;        // n_views
  uint32_t* draw_args;           // n_views x 4, or null
  uint32_t* list_stats;          // 2 + n_views, or null
};

// count, views form: grid row = view
static __global__ __launch_bounds__(kClusterThreads) __attribute__((unused)) void mip_cluster_views_list_count_kernel(const ClusterViewsListArgs a) {
  __shared__ uint32_t s_wave[kWaves];
  const uint32_t v = blockIdx.y;  // < n_views
  const unsigned long long* survive = a.v.view_words + (size_t)(1u + v) * a.v.words_stride;
  uint32_t* word_rank = a.word_rank + (size_t)v * a.rank_stride;
  uint32_t* list_tiles = a.list_tiles + (size_t)v * a.tile_stride;
  const uint32_t w_total = a.v.c.scalars[kClusterScW];
  const uint32_t n_words = cluster_survive_words(w_total), n_tiles = cluster_list_tiles(w_total);
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t tile = cluster_loop_tile(a.v.c, t, n_tiles);
    const uint32_t word = tile * kClusterListTileWords + threadIdx.x;
    const bool valid = word < n_words;  // n_words <= rank_stride, words_stride: the scan held W to the bound the planes are sized by
    uint32_t total;
    const uint32_t excl = batch_block_scan(valid ? (uint32_t)__popcll(survive[word]) : 0u, s_wave, total);
    if (valid) word_rank[word] = excl;
    if (threadIdx.x == 0u) list_tiles[tile] = total;  // tile < list tiles of W <= tile_stride
  }
}

// epilogue, views form: one workgroup per view. Several workgroups may raise the status at once: they all store the same bit
// over the same old value (the scan, the only other kernel of the call that raises, has finished).
static __global__ __launch_bounds__(kClusterThreads) __attribute__((unused)) void mip_cluster_views_list_epilogue_kernel(const ClusterViewsListArgs a) {
  __shared__ uint32_t s_wave[kWaves];
  const uint32_t v = blockIdx.x;  // < n_views
  uint32_t* list_tiles = a.list_tiles + (size_t)v * a.tile_stride;
  const uint32_t n_tiles = cluster_list_tiles(a.v.c.scalars[kClusterScW]);  // 0 when the call does not run
  uint32_t before = 0;  // survivors_v <= W < 2^32
  for (uint32_t first = 0; first < n_tiles; first += kClusterThreads) {
    const uint32_t t = first + threadIdx.x;
    uint32_t total;
    const uint32_t excl = batch_block_scan(t < n_tiles ? list_tiles[t] : 0u, s_wave, total);
    if (t < n_tiles) list_tiles[t] = before + excl;
    before += total;
  }
  if (threadIdx.x == 0u) {
    const uint32_t count = before < a.entry_stride ? before : a.entry_stride;
    a.entry_counts[v] = count;
    if (a.draw_args) {
      uint32_t* d = a.draw_args + 4u * v;
      d[0] = kClusterListDrawVertices;
      d[1] = count;
      d[2] = 0u;
      d[3] = (uint32_t)cluster_views_list_first(v, a.entry_stride);  // < 2^32: the entry point refused anything else
    }
    if (a.list_stats) {
      a.list_stats[2u + v] = before;
      if (v == 0u) {
        a.list_stats[0] = a.v.c.scalars[kClusterScWTrue];
        a.list_stats[1] = a.v.c.scalars[kClusterScMembers];
      }
    }
    if (before > a.entry_stride) cluster_raise(a.v.c, kClusterStatusCapacity);
  }
}

// write, views form: the located item and the three fields all views share once per wave and round, one store per view a lane
// survives in
static __global__ __launch_bounds__(kClusterThreads) __attribute__((unused)) void mip_cluster_views_list_write_kernel(const ClusterViewsListArgs a) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const ClusterArgs& c = a.v.c;
  const uint32_t w_total = c.scalars[kClusterScW], members = c.scalars[kClusterScMembers];
  const uint32_t n_tiles = cluster_item_tiles(w_total);
  const uint32_t n_views = a.v.n_views;
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t tile = cluster_loop_tile(c, t, n_tiles);
#pragma unroll 1
    for (uint32_t r = 0; r < kBatchRounds; ++r) {
      const unsigned long long base64 = (unsigned long long)tile * kClusterItemTile + wave * (kBatchRounds * 64u) + r * 64u;
      if (base64 >= w_total) break;  // (the whole wave; the rounds behind it start later still)
      const uint32_t base = (uint32_t)base64, word = base >> 6;
      // the per-view words, one view per lane: lane v < n_views loads view v's survive word, and the survivors of the view in
      // front of the word (tile prefix + word rank). Three loads per round in flight at once, whatever n_views, where a loop of
      // scalar loads would wait for three loads per VIEW one behind the other; the view loop reads them with readlane
      const uint32_t list_tile = word / kClusterListTileWords;
      unsigned long long mine = 0ull;
      uint32_t before_mine = 0u;
      if (lane < n_views) {
        mine = a.v.view_words[(size_t)(1u + lane) * a.v.words_stride + word];
        before_mine = a.list_tiles[(size_t)lane * a.tile_stride + list_tile] + a.word_rank[(size_t)lane * a.rank_stride + word];
      }
      if (__ballot(mine != 0ull) == 0ull) continue;  // (the whole wave: no view has a survivor among these 64 items)
      const uint32_t m0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.word_member[word]);
      const ClusterItem it = cluster_list_locate(c, m0, base, lane, w_total, members);
      uint4 e = make_uint4(0u, 0u, 0u, 0u);
      if (base + lane < w_total) {  // the three fields all views share
        const uint32_t ml = c.lods.bucket_lod[c.bucket[it.inst]];
        const uint32_t mesh = ml >> 3, lod = ml & 7u;
        const MeshChain& ch = c.lods.chain[mesh];
        e.y = ch.index_offset[lod] + kClusterIndices * it.cluster;  // the source mesh's own range
        e.z = (uint32_t)c.lods.mesh_draw[mesh].vertex_offset;
        e.w = cluster_list_index_count(it.cluster, cluster_level_triangles(ch.index_len[lod]));
      }
#pragma unroll 1
      for (uint32_t v = 0; v < n_views; ++v) {  // (uniform: v is a scalar, the words come out of lane v)
        const unsigned long long s = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(mine >> 32), (int)v) << 32) |
                                     (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)mine, (int)v);
        if (s == 0ull) continue;  // (the whole wave; the views behind it still run)
        const uint32_t before = (uint32_t)__builtin_amdgcn_readlane((int)before_mine, (int)v);
        if (before >= a.entry_stride) continue;  // (the whole wave: every rank of the word is at or above the view's stride)
        const uint32_t rank = before + lanes_below(s);
        if (((s >> lane) & 1ull) != 0ull && base + lane < w_total && rank < a.entry_stride) {
          e.x = a.v.view_base[v] + it.inst;
          a.entries[(size_t)cluster_views_list_first(v, a.entry_stride) + rank] = e;  // < n_views x entry_stride < 2^32
        }
      }
    }
  }
}

}  // namespace mip
