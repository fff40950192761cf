// cluster_list_kernel.hpp — mip_list_clusters (the visible-cluster list for one indirect draw; extension, not reference
// behaviour), gfx950: one 16-byte entry per surviving work item in place of one command per run. include/mi_instance_pipeline.h
// specifies it, tests/cluster_list_restatement.py restates it in numpy, cluster_list_plan.hpp holds the arithmetic that is not
// a kernel. Instantiated in api_cluster.hip only.
//
// The front of the call is mip_cull_clusters' (or the cone call's) own launches, unchanged: count, scan, members, cull. They
// leave {survive, start} per 64 work items in `words`. Behind them, on the same stream:
//
//   word members  one survive word per thread: word_member[k] = the member of work item 64 k (cluster_list_word_member, one
//                 search per WORD, every thread its own) — the scratch word that spares the write kernel the uniform search
//                 cluster_locate repeats per wave and round
//   count         one survive word per thread, a tile of 256 words per workgroup: popcount -> word_rank[k] = the survivors of
//                 the tile's words in front of word k; the tile's total -> list_tiles[tile]
//   epilogue      one workgroup: the tile totals become exclusive prefixes; entry_count, draw_args, stats, the overflow status;
//                 of a call the scan refused (W = 0 here) it writes the refusal: a zero count, {192, 0, 0, 0}, {0, W, members}
//   write         the cull kernel's shape: 64 work items per wave and round. A zero survive word is skipped; else word_member,
//                 the 64 member_first entries behind it one per lane, six shuffles for the lane's own member
//                 (cluster_list_locate: no search), rank = tile prefix + word rank + lanes below, and ONE 16-byte store per
//                 surviving lane below entry_capacity: the survivors of a wave write one contiguous span of at most 1 KiB
//
// No workgroup waits for another and nothing depends on the order workgroups start in; the looping grids are capped
// (cluster_list_plan.hpp) and the diagnostic build permutes their tiles.
#pragma once

#include "cluster_kernel.hpp"
#include "cluster_list_plan.hpp"

#pragma clang fp contract(off)

namespace mip {

static_assert(kClusterListTileWords == kClusterThreads, "one survive word per thread of a tile");
static_assert(kClusterListTile % kClusterItemTile == 0u, "an item tile of the write kernel lies inside one list tile");

struct ClusterListArgs {
  ClusterArgs c;                 // the front's arguments, as its kernels take them (cmds / cmd_count / stats unused)
  // scratch
  uint32_t* word_member;         // per 64 work items: the member of the word's first item
  uint32_t* word_rank;           // per 64 work items: the survivors of its list tile in front of the word
  uint32_t* list_tiles;          // list tiles: survivors, then (epilogue) the survivors of the tiles before
  // outputs
  uint4* entries;                // MipClusterEntry
  uint32_t entry_capacity;
  uint32_t* entry_count;
  uint32_t* draw_args;           // or null
  uint32_t* list_stats;          // or null
};

// word members: word_member[k] for every k < ceil(W / 64)
static __global__ __launch_bounds__(kClusterThreads) __attribute__((unused)) void mip_cluster_list_word_members_kernel(const ClusterListArgs a) {
  const uint32_t w_total = a.c.scalars[kClusterScW], members = a.c.scalars[kClusterScMembers];
  const uint32_t n_words = cluster_survive_words(w_total), n_tiles = cluster_list_tiles(w_total);
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t tile = cluster_loop_tile(a.c, t, n_tiles);
    const uint32_t word = tile * kClusterListTileWords + threadIdx.x;
    if (word < n_words) a.word_member[word] = cluster_list_word_member(a.c.member_first, members, word);  // 64 word < W
  }
}

// count: the rank of every survive word inside its tile, and the tile's survivors
static __global__ __launch_bounds__(kClusterThreads) __attribute__((unused)) void mip_cluster_list_count_kernel(const ClusterListArgs a) {
  __shared__ uint32_t s_wave[kWaves];
  const uint32_t w_total = a.c.scalars[kClusterScW];
  const uint32_t n_words = cluster_survive_words(w_total), n_tiles = cluster_list_tiles(w_total);
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t tile = cluster_loop_tile(a.c, t, n_tiles);
    const uint32_t word = tile * kClusterListTileWords + threadIdx.x;
    const bool valid = word < n_words;
    uint32_t total;
    const uint32_t excl = batch_block_scan(valid ? (uint32_t)__popcll(a.c.words[word].x) : 0u, s_wave, total);
    if (valid) a.word_rank[word] = excl;
    if (threadIdx.x == 0u) a.list_tiles[tile] = total;
  }
}

// epilogue: the tile totals become exclusive prefixes; the count, the draw arguments, the stats and the status. One workgroup.
static __global__ __launch_bounds__(kClusterThreads) __attribute__((unused)) void mip_cluster_list_epilogue_kernel(const ClusterListArgs a) {
  __shared__ uint32_t s_wave[kWaves];
  const uint32_t n_tiles = cluster_list_tiles(a.c.scalars[kClusterScW]);  // 0 when the call does not run
  uint32_t before = 0;  // survivors <= W < 2^32
  for (uint32_t first = 0; first < n_tiles; first += kClusterThreads) {
    const uint32_t t = first + threadIdx.x;
    uint32_t total;
    const uint32_t excl = batch_block_scan(t < n_tiles ? a.list_tiles[t] : 0u, s_wave, total);
    if (t < n_tiles) a.list_tiles[t] = before + excl;
    before += total;
  }
  if (threadIdx.x == 0u) {
    const uint32_t count = before < a.entry_capacity ? before : a.entry_capacity;
    *a.entry_count = count;
    // (the compiler merges the four words into one 16-byte store; a gfx950 global store takes a wide access at any 4-byte
    // aligned address, which is all the header asks of draw_args)
    if (a.draw_args) {
      a.draw_args[0] = kClusterListDrawVertices;
      a.draw_args[1] = count;
      a.draw_args[2] = 0u;
      a.draw_args[3] = 0u;
    }
    if (a.list_stats) {
      a.list_stats[0] = before;
      a.list_stats[1] = a.c.scalars[kClusterScWTrue];
      a.list_stats[2] = a.c.scalars[kClusterScMembers];
    }
    if (before > a.entry_capacity) cluster_raise(a.c, kClusterStatusCapacity);
  }
}

// cluster_locate without its search: m0 = word_member[base / 64] is the member of `base`, a multiple of 64 below W. Every
// lane finds its own member among the 64 entries behind m0 (held one per lane) with six shuffles. A lane whose item is at or
// above W locates `base` instead: its loads stay in bounds and its result is not used. Called by whole waves.
__device__ __forceinline__ ClusterItem cluster_list_locate(const ClusterArgs& a, uint32_t m0, uint32_t base, uint32_t lane, uint32_t w_total, uint32_t members) {
  const uint32_t mine = m0 + lane < members ? a.member_first[m0 + lane] : 0xffffffffu;  // strictly increasing; W < 2^32 - 1 <= the filler
  const uint32_t w = base + lane < w_total ? base + lane : base;  // (base <= 2^32 - 64: the sum does not wrap)
  uint32_t j = 0;
#pragma unroll
  for (uint32_t step = 32; step > 0; step >>= 1) {
    const uint32_t at = (uint32_t)__shfl((int)mine, (int)(j + step));  // j + step <= 63
    if (at <= w) j += step;
  }
  const uint32_t first = (uint32_t)__shfl((int)mine, (int)j);
  return {a.member_inst[m0 + j], w - first};
}

// write: one entry per surviving work item, in work-item order
static __global__ __launch_bounds__(kClusterThreads) __attribute__((unused)) void mip_cluster_list_write_kernel(const ClusterListArgs a) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t w_total = a.c.scalars[kClusterScW], members = a.c.scalars[kClusterScMembers];
  const uint32_t n_tiles = cluster_item_tiles(w_total);
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t tile = cluster_loop_tile(a.c, t, n_tiles);
#pragma unroll 1
    for (uint32_t r = 0; r < kBatchRounds; ++r) {
      const unsigned long long base64 = (unsigned long long)tile * kClusterItemTile + wave * (kBatchRounds * 64u) + r * 64u;
      if (base64 >= w_total) break;  // (the whole wave; the rounds behind it start later still)
      const uint32_t base = (uint32_t)base64, word = base >> 6;
      const unsigned long long loaded = a.c.words[word].x;
      const unsigned long long s = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(loaded >> 32)) << 32) |
                                   (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)loaded);
      if (s == 0ull) continue;  // (the whole wave)
      const uint32_t before = (uint32_t)__builtin_amdgcn_readfirstlane((int)(a.list_tiles[word / kClusterListTileWords] + a.word_rank[word]));
      if (before >= a.entry_capacity) continue;  // (the whole wave: every rank of the word is at or above the capacity)
      const uint32_t m0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.word_member[word]);
      const ClusterItem it = cluster_list_locate(a.c, m0, base, lane, w_total, members);
      const uint32_t rank = before + lanes_below(s);
      if (((s >> lane) & 1ull) != 0ull && base + lane < w_total && rank < a.entry_capacity) {
        const uint32_t ml = a.c.lods.bucket_lod[a.c.bucket[it.inst]];
        const uint32_t mesh = ml >> 3, lod = ml & 7u;
        const MeshChain& ch = a.c.lods.chain[mesh];
        uint4 e;
        e.x = a.c.lods.first_instance_base + it.inst;
        e.y = ch.index_offset[lod] + kClusterIndices * it.cluster;  // the source mesh's own range
        e.z = (uint32_t)a.c.lods.mesh_draw[mesh].vertex_offset;
        e.w = cluster_list_index_count(it.cluster, cluster_level_triangles(ch.index_len[lod]));
        a.entries[rank] = e;
      }
    }
  }
}

}  // namespace mip
