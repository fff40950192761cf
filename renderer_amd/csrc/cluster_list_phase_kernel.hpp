// cluster_list_phase_kernel.hpp — mip_list_clusters_phase (the visible-cluster list in two phases; extension, not reference
// behaviour), gfx950: mip_cull_clusters_phase's record with mip_list_clusters' entries in the commands' place, the list started
// at an entry base read on the device. include/mi_instance_pipeline.h specifies it, tests/cluster_list_phase_restatement.py
// restates it in numpy, cluster_list_phase_plan.hpp holds the arithmetic that is not a kernel. Instantiated in api_cluster.hip only.
//
// count, scan, members and word members are the kernels mip_cull_clusters_phase and mip_list_clusters launch, unchanged; word
// members stands in FRONT of the cull here, because it needs member_first alone. Behind them, on the same stream:
//
//   cull (FIRST)    the body of mip_cluster_cull_kernel<true> with cluster_list_locate(word_member[base / 64]) in
//                   cluster_locate's place: no search. The survive word and the record word are the ones that kernel stores
//   retest (SECOND) the body of mip_cluster_retest_kernel with the same swap; the zero-word shortcut and cluster_world_box stay
//                   Neither stores a start word: no list kernel reads one, so the cheapest store is none — the 8 bytes of
//                   the survive word alone; the start half of `words` keeps whatever an earlier call of the slot left there
//   count           one survive word per thread, a tile of 256 words per workgroup: word_rank and list_tiles as
//                   mip_list_clusters' count kernel; in FIRST a second row per tile, the popcounts of the record's words
//   epilogue        one workgroup: the tile prefixes; b = *entry_base (or 0) and room = entry_capacity - min(b, entry_capacity);
//                   entry_count, draw_args {192, count, 0, b}, stats {survivors, W, members, candidates}, the status bits; in
//                   FIRST the record's header; b and room to two scratch words for the write kernel. A call the scan refused
//                   (W = 0 here: a work overflow, or in SECOND a record that is not the call's) gets its zeros here
//   write           mip_list_clusters' write kernel with entries[b + rank] and rank < room: one aligned 16-byte store per
//                   survivor; a word is skipped when it is zero or its first rank — the smallest — is at or above room
//
// No workgroup waits for another and nothing depends on the order workgroups start in; the looping grids are capped
// (cluster_list_phase_plan.hpp) and the diagnostic build permutes their tiles.
#pragma once

#include "cluster_list_kernel.hpp"
#include "cluster_list_phase_plan.hpp"

#pragma clang fp contract(off)

namespace mip {

struct ClusterListPhaseArgs {
  ClusterListArgs l;             // the list's arguments, the front's inside them (l.c.record_header / record_words: the record)
  const uint32_t* entry_base;    // DEVICE, or null: the entry the list starts at
  // scratch
  uint32_t* list_candidates;     // list tiles (FIRST): the candidates of the tile's record words
  uint32_t* phase_scalars;       // kClusterListPhaseScWords: b and room, written by the epilogue
};

// cull (FIRST): both tests on every work item; the survive word and the record word of every 64
static __global__ __launch_bounds__(kClusterThreads, 4) __attribute__((unused)) void mip_cluster_list_phase_cull_kernel(const ClusterListPhaseArgs p) {
  const ClusterArgs& a = p.l.c;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t w_total = a.scalars[kClusterScW], members = a.scalars[kClusterScMembers];
  const uint32_t n_tiles = cluster_item_tiles(w_total);
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t tile = cluster_loop_tile(a, t, n_tiles);
#pragma unroll 1
    for (uint32_t r = 0; r < kBatchRounds; ++r) {
      const unsigned long long base64 = (unsigned long long)tile * kClusterItemTile + wave * (kBatchRounds * 64u) + r * 64u;
      if (base64 >= w_total) break;  // (the whole wave; the rounds behind it start later still)
      const uint32_t base = (uint32_t)base64;
      const uint32_t m0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.l.word_member[base >> 6]);
      const ClusterItem it = cluster_list_locate(a, m0, base, lane, w_total, members);
      const bool active = base + lane < w_total;
      Instance inst;
      cluster_world_box(a, it, inst);
      bool survives = active && !coarse_culled(inst, a.planes);
      const bool passed = survives;
      if (survives) survives = !box_occluded(inst.mins, inst.maxs, a.pv, a.pyramid, a.width, a.height);  // (the entry point refuses a null occ)
      const unsigned long long s = __ballot(survives);
      const unsigned long long candidates = __ballot(passed && !survives);  // (an item at or above W is not active: its bit is 0)
      if (lane == 0u) {
        a.words[base >> 6].x = s;  // no start word: nothing behind this kernel reads one
        a.record_words[base >> 6] = candidates;
      }
    }
  }
}

// retest (SECOND): the Hi-Z test alone, on the items the record names; a zero record word is a zero survive word
static __global__ __launch_bounds__(kClusterThreads, 4) __attribute__((unused)) void mip_cluster_list_phase_retest_kernel(const ClusterListPhaseArgs p) {
  const ClusterArgs& a = p.l.c;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t w_total = a.scalars[kClusterScW], members = a.scalars[kClusterScMembers];
  const uint32_t n_tiles = cluster_item_tiles(w_total);
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t tile = cluster_loop_tile(a, t, n_tiles);
#pragma unroll 1
    for (uint32_t r = 0; r < kBatchRounds; ++r) {
      const unsigned long long base64 = (unsigned long long)tile * kClusterItemTile + wave * (kBatchRounds * 64u) + r * 64u;
      if (base64 >= w_total) break;  // (the whole wave; the rounds behind it start later still)
      const uint32_t base = (uint32_t)base64;
      const unsigned long long loaded = a.record_words[base >> 6];  // word < ceil(W / 64): the scan matched W, the host the room
      const unsigned long long candidates = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(loaded >> 32)) << 32) |
                                            (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)loaded);
      if (candidates == 0ull) {  // (the whole wave)
        if (lane == 0u) a.words[base >> 6].x = 0ull;
        continue;
      }
      const uint32_t m0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.l.word_member[base >> 6]);
      const ClusterItem it = cluster_list_locate(a, m0, base, lane, w_total, members);
      const bool active = base + lane < w_total && ((candidates >> lane) & 1ull) != 0ull;
      Instance inst;
      cluster_world_box(a, it, inst);
      const bool survives = active && !box_occluded(inst.mins, inst.maxs, a.pv, a.pyramid, a.width, a.height);
      const unsigned long long s = __ballot(survives);
      if (lane == 0u) a.words[base >> 6].x = s;
    }
  }
}

// count: the rank of every survive word inside its tile and the tile's survivors; kFirst: and the tile's candidates
template <bool kFirst>
__global__ __launch_bounds__(kClusterThreads) void mip_cluster_list_phase_count_kernel(const ClusterListPhaseArgs p) {
  __shared__ uint32_t s_wave[kWaves];
  const ClusterArgs& a = p.l.c;
  const uint32_t w_total = a.scalars[kClusterScW];
  const uint32_t n_words = cluster_survive_words(w_total), n_tiles = cluster_list_tiles(w_total);
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t tile = cluster_loop_tile(a, t, n_tiles);
    const uint32_t word = tile * kClusterListTileWords + threadIdx.x;
    const bool valid = word < n_words;
    uint32_t total;
    const uint32_t excl = batch_block_scan(valid ? (uint32_t)__popcll(a.words[word].x) : 0u, s_wave, total);
    if (valid) p.l.word_rank[word] = excl;
    if (threadIdx.x == 0u) p.l.list_tiles[tile] = total;
    if constexpr (kFirst) {
      uint32_t candidates;
      (void)batch_block_scan(valid ? (uint32_t)__popcll(a.record_words[word]) : 0u, s_wave, candidates);
      if (threadIdx.x == 0u) p.list_candidates[tile] = candidates;
    }
  }
}

// epilogue: the tile prefixes; the base and the room; the count, the draw arguments, the stats, the status; kFirst: the header
template <bool kFirst>
__global__ __launch_bounds__(kClusterThreads) void mip_cluster_list_phase_epilogue_kernel(const ClusterListPhaseArgs p) {
  __shared__ uint32_t s_wave[kWaves];
  const ClusterArgs& a = p.l.c;
  const uint32_t n_tiles = cluster_list_tiles(a.scalars[kClusterScW]);  // 0 when the call does not run
  uint32_t before = 0;  // survivors <= W < 2^32
  uint32_t candidates = 0;
  for (uint32_t first = 0; first < n_tiles; first += kClusterThreads) {
    const uint32_t t = first + threadIdx.x;
    uint32_t total;
    if constexpr (kFirst) {
      (void)batch_block_scan(t < n_tiles ? p.list_candidates[t] : 0u, s_wave, total);
      candidates += total;
    }
    const uint32_t excl = batch_block_scan(t < n_tiles ? p.l.list_tiles[t] : 0u, s_wave, total);
    if (t < n_tiles) p.l.list_tiles[t] = before + excl;
    before += total;
  }
  if (threadIdx.x == 0u) {
    const bool runs = a.scalars[kClusterScRuns] != 0u;
    if constexpr (!kFirst) candidates = runs ? a.record_header[2] : 0u;  // the header's word, as FIRST wrote it
    const uint32_t b = p.entry_base ? *p.entry_base : 0u;  // read before anything is written (the entry point refuses an alias anyway)
    const uint32_t room = cluster_list_phase_room(b, p.l.entry_capacity);
    const uint32_t count = before < room ? before : room;
    p.phase_scalars[kClusterListPhaseScBase] = b;
    p.phase_scalars[kClusterListPhaseScRoom] = room;
    *p.l.entry_count = count;
    if (p.l.draw_args) {
      p.l.draw_args[0] = kClusterListDrawVertices;
      p.l.draw_args[1] = count;
      p.l.draw_args[2] = 0u;
      p.l.draw_args[3] = b;
    }
    if (p.l.list_stats) {
      p.l.list_stats[0] = before;
      p.l.list_stats[1] = a.scalars[kClusterScWTrue];
      p.l.list_stats[2] = a.scalars[kClusterScMembers];
      p.l.list_stats[3] = candidates;
    }
    if (before > room) cluster_raise(a, kClusterStatusCapacity);
    if constexpr (kFirst) {
      a.record_header[0] = runs ? a.scalars[kClusterScW] : kClusterRecordRefused;
      a.record_header[1] = runs ? a.scalars[kClusterScMembers] : 0u;
      a.record_header[2] = runs ? candidates : 0u;
      a.record_header[3] = 0u;
    }
  }
}

// write: one entry per surviving work item, in work-item order, from entry b
static __global__ __launch_bounds__(kClusterThreads) __attribute__((unused)) void mip_cluster_list_phase_write_kernel(const ClusterListPhaseArgs p) {
  const ClusterArgs& a = p.l.c;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t w_total = a.scalars[kClusterScW], members = a.scalars[kClusterScMembers];
  const uint32_t b = p.phase_scalars[kClusterListPhaseScBase], room = p.phase_scalars[kClusterListPhaseScRoom];  // b + room <= entry_capacity when room > 0
  const uint32_t n_tiles = cluster_item_tiles(w_total);
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t tile = cluster_loop_tile(a, t, n_tiles);
#pragma unroll 1
    for (uint32_t r = 0; r < kBatchRounds; ++r) {
      const unsigned long long base64 = (unsigned long long)tile * kClusterItemTile + wave * (kBatchRounds * 64u) + r * 64u;
      if (base64 >= w_total) break;  // (the whole wave; the rounds behind it start later still)
      const uint32_t base = (uint32_t)base64, word = base >> 6;
      const unsigned long long loaded = a.words[word].x;
      const unsigned long long s = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(loaded >> 32)) << 32) |
                                   (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)loaded);
      if (s == 0ull) continue;  // (the whole wave)
      const uint32_t before = (uint32_t)__builtin_amdgcn_readfirstlane((int)(p.l.list_tiles[word / kClusterListTileWords] + p.l.word_rank[word]));
      if (before >= room) continue;  // (the whole wave: the word's first rank, and so every rank of it, is at or above the room)
      const uint32_t m0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.l.word_member[word]);
      const ClusterItem it = cluster_list_locate(a, m0, base, lane, w_total, members);
      const uint32_t rank = before + lanes_below(s);
      if (((s >> lane) & 1ull) != 0ull && base + lane < w_total && rank < room) {
        const uint32_t ml = a.lods.bucket_lod[a.bucket[it.inst]];
        const uint32_t mesh = ml >> 3, lod = ml & 7u;
        const MeshChain& ch = a.lods.chain[mesh];
        uint4 e;
        e.x = a.lods.first_instance_base + it.inst;
        e.y = ch.index_offset[lod] + kClusterIndices * it.cluster;  // the source mesh's own range
        e.z = (uint32_t)a.lods.mesh_draw[mesh].vertex_offset;
        e.w = cluster_list_index_count(it.cluster, cluster_level_triangles(ch.index_len[lod]));
        p.l.entries[(size_t)b + rank] = e;  // b + rank < b + room = entry_capacity
      }
    }
  }
}

}  // namespace mip
