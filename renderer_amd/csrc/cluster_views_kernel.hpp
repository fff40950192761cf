// cluster_views_kernel.hpp — cluster culling for several views in one call (mip_cull_clusters_views; extension, not reference
// behaviour), gfx950. include/mi_instance_pipeline.h specifies it, tests/cluster_views_restatement.py restates it in numpy,
// cluster_views_plan.hpp holds the arithmetic that is not a kernel. Instantiated in api_cluster.hip only.
//
// One LOD for all views (frames[0].cam_pos) makes a work item (i, c), and its world box, common to every view: everything the
// plain cull kernel does in front of its plane test is done once per work item, and only the six planes and the bitmap bit
// differ per view. Seven launches on the context's first stream, whatever n_views:
//
//   count      views form: one read of every view's bitmap word per instance -> a 16-bit view mask per instance (view_mask);
//              items(i) = C(bucket) iff the mask is non-zero and T > 0, the level from frames[0].cam_pos by lod_chain_pick
//   scan       cluster_kernel.hpp's, the plain instantiation, unchanged: its argument block is the leading part of this one
//   members    cluster_kernel.hpp's, unchanged
//   cull       views form, the hot path: per wave of 64 items cluster_locate, the loads, quat_to_rotation and instance_tiered
//              ONCE; then a uniform loop over the views: a lane is live iff its item is below W and bit v of its instance's
//              mask is set; view v's 24 plane floats are wave-uniform and come from the argument block by scalar loads;
//              ballot -> view v's survive word. No live lane: a zero word and no plane arithmetic (a wave-uniform branch).
//              The start word is stored once per 64 items
//   heads      views form: grid row = view; cluster_head_mask's word arithmetic on view v's plane of survive words
//   epilogue   views form: one workgroup per view: the view's head counts become exclusive prefixes; cmd_counts[v], the
//              view's two stats words, the status; the workgroup of view 0 also writes W and members
//   commands   views form: grid row = view; the plain kernel's body on view v's words, into v * cmd_stride, stops at cmd_stride
//
// Scratch: (1 + n_views) x 8 bytes per 64 work items of the bound — plane 0 the start words, plane 1 + v view v's survive
// words — and 2 bytes per instance, beside what the plain call takes per instance and per tile.
// An instance outside view v's bitmap has no survivor in view v, so it has no head and no command there, and a run of view v
// never reaches into it (a run never crosses an instance: the start bit): view v's commands are those of a plain call over
// view v's bitmap alone, byte for byte.
// The uniform binary search of cluster_locate is kept (cull once per 64 items, commands once per word with a head and view):
// DESIGN's "word-member scratch word" is not built here.
#pragma once

#include "cluster_kernel.hpp"
#include "cluster_views_plan.hpp"

#pragma clang fp contract(off)

namespace mip {

static_assert(kClusterMaxViews == MIP_MAX_VIEWS && kClusterMaxViews <= 16u, "a view is a bit of the 16-bit mask");

struct ClusterViewArgs {
  // what scan and members read, and the fields the views kernels share with the plain ones. Not read of it: lods.bitmap,
  // lods.first_instance_base, planes, pv, pyramid, words, the record. cmds = view 0's first entry, cmd_capacity = cmd_stride,
  // cmd_count = cmd_counts, stats = the 2 + 2 n_views words or null, tile_heads / tile_survivors = n_views rows.
  ClusterArgs c;
  uint32_t n_views;
  uint32_t head_tiles;                       // entries of a row of tile_heads / tile_survivors
  unsigned long long words_stride;           // entries of a plane of view_words
  unsigned long long* view_words;            // plane 0: start words; plane 1 + v: view v's survive words
  uint16_t* view_mask;                       // n: bit v set <=> instance i's bit is set in view v's bitmap
  const uint32_t* view_bitmap[kClusterMaxViews];  // null: every resident instance
  uint32_t view_base[kClusterMaxViews];      // first_instance_base of every view
  float view_planes[kClusterMaxViews][24];
};

// count, views form
template <uint32_t kMode>
__global__ __launch_bounds__(kClusterThreads) void mip_cluster_views_count_kernel(const ClusterViewArgs a) {
  __shared__ unsigned long long s_items[kWaves];
  __shared__ uint32_t s_members[kWaves];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t tile = batch_tile(a.c.lods);
  const uint32_t n = a.c.lods.n;
  unsigned long long items = 0;
  uint32_t members = 0;
#pragma unroll
  for (uint32_t r = 0; r < kBatchRounds; ++r) {
    const uint32_t idx = batch_index(tile, wave, r, lane);
    const bool active = idx < n;
    const uint32_t il = active ? idx : n - 1u;  // an idle lane loads the last instance, in bounds
    uint32_t mask = 0;
#pragma unroll 1
    for (uint32_t v = 0; v < a.n_views; ++v) {  // (uniform: the pointer is a scalar load)
      const uint32_t* bitmap = a.view_bitmap[v];
      const uint32_t word = bitmap ? bitmap[il >> 5] : 0xffffffffu;
      mask |= ((word >> (il & 31u)) & 1u) << v;
    }
    // the union's bit in the place of a bitmap word; the reference point is frames[0]'s
    const LodChainPick s = lod_chain_pick<kMode>(a.c.lods, il, active, mask ? 0xffffffffu : 0u, a.c.lods.cam[0], a.c.lods.cam[1], a.c.lods.cam[2]);
    const uint32_t c = s.member ? a.c.cluster_base[s.bucket + 1u] - a.c.cluster_base[s.bucket] : 0u;
    if (active) {
      a.c.items[idx] = c;
      a.c.bucket[idx] = s.bucket;
      a.view_mask[idx] = (uint16_t)mask;
    }
    items += (unsigned long long)wave_sum(c & 0xffffu) + ((unsigned long long)wave_sum(c >> 16) << 16);  // C < 2^31: neither half sum wraps
    members += (uint32_t)__popcll(__ballot(c != 0u));
  }
  if (lane == 0u) {
    s_items[wave] = items;
    s_members[wave] = members;
  }
  __syncthreads();
  if (threadIdx.x == 0u) {
    unsigned long long ti = 0;
    uint32_t tm = 0;
#pragma unroll
    for (uint32_t w = 0; w < kWaves; ++w) {
      ti += s_items[w];
      tm += s_members[w];
    }
    a.c.tile_items[tile] = ti;
    a.c.tile_members[tile] = tm;
  }
}

// cull, views form: the world box once per work item, the plane test once per view with a live lane
static __global__ __launch_bounds__(kClusterThreads, 4) __attribute__((unused)) void mip_cluster_views_cull_kernel(const ClusterViewArgs a) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t w_total = a.c.scalars[kClusterScW], members = a.c.scalars[kClusterScMembers];
  const uint32_t n_tiles = cluster_item_tiles(w_total);
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t tile = cluster_loop_tile(a.c, t, n_tiles);
#pragma unroll 1
    for (uint32_t r = 0; r < kBatchRounds; ++r) {
      const unsigned long long base64 = (unsigned long long)tile * kClusterItemTile + wave * (kBatchRounds * 64u) + r * 64u;
      if (base64 >= w_total) break;  // (the whole wave; the rounds behind it start later still)
      const uint32_t base = (uint32_t)base64;
      const ClusterItem it = cluster_locate(a.c, base, lane, w_total, members);
      const bool active = base + lane < w_total;
      Instance inst;
      cluster_world_box(a.c, it, inst);
      const uint32_t mask = active ? (uint32_t)a.view_mask[it.inst] : 0u;
      const size_t word = base >> 6;  // < ceil(W / 64) <= words_stride: the scan held W to the bound the planes are sized by
      const unsigned long long start = __ballot(active && it.cluster == 0u);
      if (lane == 0u) a.view_words[word] = start;
#pragma unroll 1
      for (uint32_t v = 0; v < a.n_views; ++v) {
        const bool live = ((mask >> v) & 1u) != 0u;
        unsigned long long s = 0ull;
        if (__ballot(live) != 0ull)  // (the whole wave)
          s = __ballot(live && !coarse_culled(inst, a.view_planes[v]));
        if (lane == 0u) a.view_words[(size_t)(1u + v) * a.words_stride + word] = s;
      }
    }
  }
}

// The heads of view v among the 64 work items of a word (cluster_head_mask over the view's plane).
__device__ __forceinline__ unsigned long long cluster_views_head_mask(const unsigned long long* survive, const unsigned long long* start, uint32_t word) {
  const unsigned long long s = survive[word];
  const unsigned long long before = word ? survive[word - 1u] >> 63 : 0ull;  // read by this thread itself
  return s & (start[word] | ~((s << 1) | before));
}

// heads, views form: grid row = view
static __global__ __launch_bounds__(kClusterThreads) __attribute__((unused)) void mip_cluster_views_heads_kernel(const ClusterViewArgs a) {
  __shared__ uint32_t s_heads[kWaves], s_survivors[kWaves];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t v = blockIdx.y;  // < n_views
  const unsigned long long* survive = a.view_words + (size_t)(1u + v) * a.words_stride;
  uint32_t* tile_heads = a.c.tile_heads + (size_t)v * a.head_tiles;
  uint32_t* tile_survivors = a.c.tile_survivors + (size_t)v * a.head_tiles;
  const uint32_t w_total = a.c.scalars[kClusterScW];
  const uint32_t n_words = cluster_survive_words(w_total), n_tiles = cluster_head_tiles(w_total);
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t tile = cluster_loop_tile(a.c, t, n_tiles);
    const uint32_t word = tile * kClusterHeadTileWords + threadIdx.x;
    const bool valid = word < n_words;
    const uint32_t heads = wave_sum(valid ? (uint32_t)__popcll(cluster_views_head_mask(survive, a.view_words, word)) : 0u);
    const uint32_t survivors = wave_sum(valid ? (uint32_t)__popcll(survive[word]) : 0u);
    if (lane == 0u) {
      s_heads[wave] = heads;
      s_survivors[wave] = survivors;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
      uint32_t th = 0, ts = 0;
#pragma unroll
      for (uint32_t w = 0; w < kWaves; ++w) {
        th += s_heads[w];
        ts += s_survivors[w];
      }
      tile_heads[tile] = th;  // tile < head tiles of W <= head_tiles: the row is sized for the bound
      tile_survivors[tile] = ts;
    }
    __syncthreads();  // the sums are free for the next tile
  }
}

// epilogue, views form: one workgroup per view: the view's head counts become exclusive prefixes; its count, its stats and the
// status. Several workgroups may raise the status at once: they all store the same bit over the same old value (the scan, the
// only other kernel of the call that raises, has finished), so whichever store lands last leaves the same word.
static __global__ __launch_bounds__(kClusterThreads) __attribute__((unused)) void mip_cluster_views_epilogue_kernel(const ClusterViewArgs a) {
  __shared__ uint32_t s_wave[kWaves];
  const uint32_t n_tiles = cluster_head_tiles(a.c.scalars[kClusterScW]);  // 0 when the call does not run
  bool overflow = false;
  const uint32_t v = blockIdx.x;  // < n_views
  {
    uint32_t* tile_heads = a.c.tile_heads + (size_t)v * a.head_tiles;
    const uint32_t* tile_survivors = a.c.tile_survivors + (size_t)v * a.head_tiles;
    uint32_t heads_before = 0, survivors = 0;
    for (uint32_t first = 0; first < n_tiles; first += kClusterThreads) {
      const uint32_t t = first + threadIdx.x;
      uint32_t th, ts;
      const uint32_t excl = batch_block_scan(t < n_tiles ? tile_heads[t] : 0u, s_wave, th);
      (void)batch_block_scan(t < n_tiles ? tile_survivors[t] : 0u, s_wave, ts);
      if (t < n_tiles) tile_heads[t] = heads_before + excl;
      heads_before += th;
      survivors += ts;
    }
    if (threadIdx.x == 0u) {
      a.c.cmd_count[v] = heads_before < a.c.cmd_capacity ? heads_before : a.c.cmd_capacity;
      if (a.c.stats) {
        a.c.stats[2u + 2u * v] = heads_before;
        a.c.stats[3u + 2u * v] = survivors;
      }
      overflow = overflow || heads_before > a.c.cmd_capacity;
    }
  }
  if (threadIdx.x == 0u) {
    if (a.c.stats && v == 0u) {
      a.c.stats[0] = a.c.scalars[kClusterScWTrue];
      a.c.stats[1] = a.c.scalars[kClusterScMembers];
    }
    if (overflow) cluster_raise(a.c, kClusterStatusCapacity);
  }
}

// commands, views form: grid row = view; one command per head of the view, in work-item order, from entry v * cmd_stride
static __global__ __launch_bounds__(kClusterThreads) __attribute__((unused)) void mip_cluster_views_commands_kernel(const ClusterViewArgs a) {
  __shared__ uint32_t s_wave[kWaves];
  __shared__ uint32_t s_rank[kClusterHeadTileWords];
  __shared__ unsigned long long s_mask[kClusterHeadTileWords];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t v = blockIdx.y;  // < n_views
  const unsigned long long* survive = a.view_words + (size_t)(1u + v) * a.words_stride;
  const uint32_t* tile_heads = a.c.tile_heads + (size_t)v * a.head_tiles;
  uint32_t* cmds = a.c.cmds + (size_t)v * a.c.cmd_capacity * kCmdWords;
  const uint32_t first_instance_base = a.view_base[v];
  const uint32_t w_total = a.c.scalars[kClusterScW], members = a.c.scalars[kClusterScMembers];
  const uint32_t n_words = cluster_survive_words(w_total), n_tiles = cluster_head_tiles(w_total);
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t tile = cluster_loop_tile(a.c, t, n_tiles);
    {
      const uint32_t word = tile * kClusterHeadTileWords + threadIdx.x;
      const unsigned long long mask = word < n_words ? cluster_views_head_mask(survive, a.view_words, word) : 0ull;
      uint32_t unused_total;
      const uint32_t excl = batch_block_scan((uint32_t)__popcll(mask), s_wave, unused_total);
      s_rank[threadIdx.x] = tile_heads[tile] + excl;  // the view's heads in front of this word (epilogue: the tiles before)
      s_mask[threadIdx.x] = mask;
    }
    __syncthreads();
#pragma unroll 1
    for (uint32_t j = 0; j < 64u; ++j) {
      const uint32_t local = wave * 64u + j;
      const unsigned long long stored = s_mask[local];
      const unsigned long long mask = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(stored >> 32)) << 32) |
                                      (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)stored);
      if (mask == 0ull) continue;  // (the whole wave)
      const uint32_t base = (tile * kClusterHeadTileWords + local) * 64u;  // < W: the word holds a survivor
      const ClusterItem it = cluster_locate(a.c, base, lane, w_total, members);
      const uint32_t rank = s_rank[local] + lanes_below(mask);
      if (((mask >> lane) & 1ull) != 0ull && rank < a.c.cmd_capacity) {  // cmd_capacity = cmd_stride: the view's range ends there
        const uint32_t ml = a.c.lods.bucket_lod[a.c.bucket[it.inst]];
        const uint32_t mesh = ml >> 3, lod = ml & 7u;
        const MeshChain& ch = a.c.lods.chain[mesh];
        const uint32_t tris = cluster_level_triangles(ch.index_len[lod]);
        const uint32_t limit = cluster_level_clusters(ch.index_len[lod]) - it.cluster;  // clusters the instance has left, this one included
        // the run: this survivor and the view's survivors straight behind it, inside the instance
        uint32_t run = 0, at = base + lane;
        while (run < limit) {
          const uint32_t bit = at & 63u, room = 64u - bit;
          const unsigned long long rest = ~(survive[at >> 6] >> bit);  // the shift brings zeros in: a clear bit below `room`, unless bit == 0
          const uint32_t ones = rest ? (uint32_t)__builtin_ctzll(rest) : 64u;
          const uint32_t take = ones < limit - run ? ones : limit - run;
          run += take;
          at += take;
          if (ones < room) break;  // a cluster that does not survive in this view ends the run
        }
        uint32_t* o = cmds + (size_t)rank * kCmdWords;
        o[0] = cluster_run_index_count(it.cluster, run, tris);
        o[1] = 1u;
        o[2] = ch.index_offset[lod] + kClusterIndices * it.cluster;  // the source mesh's own range
        o[3] = (uint32_t)a.c.lods.mesh_draw[mesh].vertex_offset;
        o[4] = first_instance_base + it.inst;
      }
    }
    __syncthreads();  // s_rank / s_mask are free for the next tile
  }
}

}  // namespace mip
