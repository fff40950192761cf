// cluster_triangle_list_kernel.hpp — mip_list_cluster_triangles (per-triangle masks on the visible-cluster list; extension,
// not reference behaviour), gfx950: mip_list_clusters' entries for the surviving work items that keep at least one triangle,
// and beside every entry the 64-bit word of the per-triangle stage's test over its cluster. include/mi_instance_pipeline.h
// specifies it, tests/cluster_triangle_list_restatement.py restates it in numpy, cluster_triangle_list_plan.hpp holds the
// arithmetic that is not a kernel. Instantiated in api_cluster.hip only.
//
// The front of the call is mip_list_clusters' own launches, unchanged: count, scan, members, cull (or the cone cull), and
// that call's word members (word_member[k] = the member of work item 64 k). Behind them, on the same stream:
//
//   test      mip_cluster_triangle_test_kernel's walk — one wave per survive word, the index triple of the NEXT item in flight
//             under this item's gathers and test, no memory operation in a branch — with the items located through
//             cluster_list_locate (word_member and six shuffles, no search). Lane k keeps the TRIANGLE WORD of item k (8 bytes
//             per item of scratch); the wave stores the NON-EMPTY word of its 64 items, the ballot of `triangle word != 0`
//             over the surviving lanes (zero for a zero survive word); the tile's surviving and tested triangles ->
//             tile_kept / tile_tested
//   count     the list's count over the non-empty words: word_rank[k] = the entries of the list tile in front of word k, the
//             tile's entries -> list_tiles; beside it the tile's surviving clusters (the popcount of the survive words) ->
//             tile_clusters
//   epilogue  one workgroup: the tile totals become exclusive prefixes; 64-bit sums of the tiles' surviving and tested
//             triangles; entry_count, draw_args, the six stats, the overflow status; of a call the scan refused (W = 0 here)
//             the refusal: a zero count, {192, 0, 0, 0}, {0, 0, W, members, 0, 0}
//   write     the list write kernel's shape with the non-empty word in the survive word's place: per lane whose bit is set
//             and whose rank is below entry_capacity ONE aligned 16-byte entry store and ONE 8-byte mask store at the same rank
//
// No workgroup waits for another and nothing depends on the order workgroups start in; the looping grids are capped
// (cluster_triangle_list_plan.hpp) and take cluster_loop_tile in the diagnostic build.
#pragma once

#include "cluster_list_kernel.hpp"
#include "cluster_triangle_kernel.hpp"
#include "cluster_triangle_list_plan.hpp"

#pragma clang fp contract(off)

namespace mip {

struct ClusterTriangleListArgs {
  ClusterListArgs l;                // mip_list_clusters' block: the front and the word members take it as it is
  const float* vertices;
  const uint32_t* indices;
  unsigned long long vertex_bytes;  // the uploaded positions (read through a bounded descriptor)
  uint32_t geometry_finite;         // every uploaded position is finite: an affine matrix may take triangle_test<true>
  float pv[16];                     // the frame's
  // scratch
  unsigned long long* triangle_words;  // per work item (written for the surviving ones only)
  unsigned long long* nonempty;     // per 64 work items: the surviving items whose triangle word is not zero
  uint32_t* tile_kept;              // per item tile: surviving triangles
  uint32_t* tile_tested;            //                triangles tested
  uint32_t* tile_clusters;          // per list tile: surviving clusters
  // outputs (entries, entry_capacity, entry_count, draw_args and the six stats words are l's)
  unsigned long long* masks;
};

// test: the triangle word of every surviving item; the non-empty word of every 64; the totals of every item tile
__global__ __launch_bounds__(kClusterThreads, 4) void mip_cluster_triangle_list_test_kernel(const ClusterTriangleListArgs ta) {
  __shared__ uint32_t s_kept[kWaves], s_tested[kWaves];
  const ClusterArgs& a = ta.l.c;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t w_total = a.scalars[kClusterScW], members = a.scalars[kClusterScMembers];
  const uint32_t n_tiles = cluster_item_tiles(w_total);
  float pv[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) pv[k] = ta.pv[k];
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t tile = cluster_loop_tile(a, t, n_tiles);
    uint32_t kept = 0, tested = 0;  // of this wave's words of the tile (wave-uniform)
#pragma unroll 1
    for (uint32_t r = 0; r < kBatchRounds; ++r) {
      const unsigned long long base64 = (unsigned long long)tile * kClusterItemTile + wave * (kBatchRounds * 64u) + r * 64u;
      if (base64 >= w_total) break;  // (the whole wave; the rounds behind it start later still)
      const uint32_t base = (uint32_t)base64, word = base >> 6;
      const unsigned long long survive = cluster_uniform64(a.words[word].x);
      unsigned long long nonempty = 0ull;
      if (survive != 0ull) {  // (the whole wave)
        const uint32_t m0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)ta.l.word_member[word]);
        const ClusterItem it = cluster_list_locate(a, m0, base, lane, w_total, members);
        float mine[16];
        cluster_item_model(a, it.inst, mine);
        const ClusterSource src = cluster_source(a, it);
        // mip_cluster_triangle_test_kernel's walk: the index triple of the NEXT item is in flight under this item's gathers and
        // test, and no memory operation stands in a branch; the last item reads its own triple again (in bounds, never used).
        auto load_triple = [&](uint32_t item) {  // the cluster's own triangles: a lane at or behind its count reads zeros — vertex 0
          const __amdgpu_buffer_rsrc_t idx = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(ta.indices) + cluster_lane_word(src.first_index, item), 0,
                                                                               (int)(cluster_lane_word(src.triangles, item) * 12u), 0x00020000);
          return __builtin_amdgcn_raw_buffer_load_b96(idx, (int)times12(lane), 0, 0);
        };
        unsigned long long rest = survive, mine_word = 0ull;
        uint32_t k = (uint32_t)__builtin_ctzll(rest);  // a surviving item: below W
        tri_u32x3 next = load_triple(k);
        while (rest != 0ull) {
          rest &= rest - 1ull;
          const tri_u32x3 i = next;
          const unsigned long long vertex_first = 12ull * cluster_lane_word(src.vertex_offset, k);
          const unsigned long long vertex_left = vertex_first < ta.vertex_bytes ? ta.vertex_bytes - vertex_first : 0ull;
          const __amdgpu_buffer_rsrc_t vtx = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<char*>(const_cast<float*>(ta.vertices)) + vertex_first, 0,
              (int)(vertex_left < kTriRegionMax ? (uint32_t)vertex_left : kTriRegionMax), 0x00020000);  // the mesh's own positions
          const tri_u32x3 v0 = __builtin_amdgcn_raw_buffer_load_b96(vtx, (int)times12(i.x), 0, 0);
          const tri_u32x3 v1 = __builtin_amdgcn_raw_buffer_load_b96(vtx, (int)times12(i.y), 0, 0);
          const tri_u32x3 v2 = __builtin_amdgcn_raw_buffer_load_b96(vtx, (int)times12(i.z), 0, 0);
          const uint32_t k_next = rest != 0ull ? (uint32_t)__builtin_ctzll(rest) : k;
          next = load_triple(k_next);
          float model[16];
#pragma unroll
          for (int e = 0; e < 16; ++e) model[e] = cluster_lane_word(mine[e], k);
          const uint32_t tris = cluster_lane_word(src.triangles, k);
          const float v[9] = {__uint_as_float(v0.x), __uint_as_float(v0.y), __uint_as_float(v0.z), __uint_as_float(v1.x), __uint_as_float(v1.y),
                              __uint_as_float(v1.z), __uint_as_float(v2.x), __uint_as_float(v2.y), __uint_as_float(v2.z)};
          const bool culled = model_is_affine(model, ta.geometry_finite) ? triangle_test<true>(model, pv, v) : triangle_test<false>(model, pv, v);  // wave-uniform
          const unsigned long long mask = __ballot(!culled && lane < tris);
          mine_word = lane == k ? mask : mine_word;
          kept += (uint32_t)__popcll(mask);
          tested += tris;
          k = k_next;
        }
        if (((survive >> lane) & 1ull) != 0ull) ta.triangle_words[base + lane] = mine_word;  // a surviving item is below W
        nonempty = __ballot(mine_word != 0ull);  // (mine_word is zero in a lane that does not survive)
      }
      if (lane == 0u) ta.nonempty[word] = nonempty;
    }
    if (lane == 0u) {
      s_kept[wave] = kept;
      s_tested[wave] = tested;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
      uint32_t tk = 0, tt = 0;  // at most 1 024 x 64 each
#pragma unroll
      for (uint32_t w = 0; w < kWaves; ++w) {
        tk += s_kept[w];
        tt += s_tested[w];
      }
      ta.tile_kept[tile] = tk;
      ta.tile_tested[tile] = tt;
    }
    __syncthreads();  // the sums are free for the next tile
  }
}

// count: the rank of every non-empty word inside its list tile, the tile's entries and the tile's surviving clusters
static __global__ __launch_bounds__(kClusterThreads) __attribute__((unused)) void mip_cluster_triangle_list_count_kernel(const ClusterTriangleListArgs ta) {
  __shared__ uint32_t s_wave[kWaves];
  const ClusterArgs& a = ta.l.c;
  const uint32_t w_total = a.scalars[kClusterScW];
  const uint32_t n_words = cluster_survive_words(w_total), n_tiles = cluster_list_tiles(w_total);
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t tile = cluster_loop_tile(a, t, n_tiles);
    const uint32_t word = tile * kClusterListTileWords + threadIdx.x;
    const bool valid = word < n_words;
    uint32_t total, clusters;
    const uint32_t excl = batch_block_scan(valid ? (uint32_t)__popcll(ta.nonempty[word]) : 0u, s_wave, total);
    (void)batch_block_scan(valid ? (uint32_t)__popcll(a.words[word].x) : 0u, s_wave, clusters);
    if (valid) ta.l.word_rank[word] = excl;
    if (threadIdx.x == 0u) {
      ta.l.list_tiles[tile] = total;
      ta.tile_clusters[tile] = clusters;
    }
  }
}

// epilogue: the tile totals become exclusive prefixes; the count, the draw arguments, the six stats and the status. One workgroup.
static __global__ __launch_bounds__(kClusterThreads) __attribute__((unused)) void mip_cluster_triangle_list_epilogue_kernel(const ClusterTriangleListArgs ta) {
  __shared__ uint32_t s_wave[kWaves];
  __shared__ unsigned long long s_scan[kClusterThreads];
  const ClusterArgs& a = ta.l.c;
  const uint32_t w_total = a.scalars[kClusterScW];  // 0 when the call does not run
  const uint32_t list_tiles = cluster_list_tiles(w_total), item_tiles = cluster_item_tiles(w_total);
  uint32_t before = 0, clusters = 0;  // entries <= surviving clusters <= W < 2^32
  for (uint32_t first = 0; first < list_tiles; first += kClusterThreads) {
    const uint32_t t = first + threadIdx.x;
    uint32_t total, tc;
    const uint32_t excl = batch_block_scan(t < list_tiles ? ta.l.list_tiles[t] : 0u, s_wave, total);
    (void)batch_block_scan(t < list_tiles ? ta.tile_clusters[t] : 0u, s_wave, tc);
    if (t < list_tiles) ta.l.list_tiles[t] = before + excl;
    before += total;
    clusters += tc;
  }
  unsigned long long kept = 0, tested = 0;  // W x 64 does not fit 32 bits
  for (uint32_t first = 0; first < item_tiles; first += kClusterThreads) {
    const uint32_t t = first + threadIdx.x;
    unsigned long long tk, tt;
    (void)cluster_block_scan64(t < item_tiles ? ta.tile_kept[t] : 0u, s_scan, tk);
    (void)cluster_block_scan64(t < item_tiles ? ta.tile_tested[t] : 0u, s_scan, tt);
    kept += tk;
    tested += tt;
  }
  if (threadIdx.x == 0u) {
    const uint32_t count = before < ta.l.entry_capacity ? before : ta.l.entry_capacity;
    *ta.l.entry_count = count;
    if (ta.l.draw_args) {
      ta.l.draw_args[0] = kClusterListDrawVertices;
      ta.l.draw_args[1] = count;
      ta.l.draw_args[2] = 0u;
      ta.l.draw_args[3] = 0u;
    }
    if (ta.l.list_stats) {
      ta.l.list_stats[0] = before;
      ta.l.list_stats[1] = clusters;
      ta.l.list_stats[2] = a.scalars[kClusterScWTrue];
      ta.l.list_stats[3] = a.scalars[kClusterScMembers];
      ta.l.list_stats[4] = (uint32_t)kept;
      ta.l.list_stats[5] = (uint32_t)tested;
    }
    if (before > ta.l.entry_capacity) cluster_raise(a, kClusterStatusCapacity);
  }
}

// write: one entry and one mask per surviving work item with a non-zero triangle word, in work-item order
static __global__ __launch_bounds__(kClusterThreads) __attribute__((unused)) void mip_cluster_triangle_list_write_kernel(const ClusterTriangleListArgs ta) {
  const ClusterArgs& a = ta.l.c;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t w_total = a.scalars[kClusterScW], members = a.scalars[kClusterScMembers];
  const uint32_t n_tiles = cluster_item_tiles(w_total);
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t tile = cluster_loop_tile(a, t, n_tiles);
#pragma unroll 1
    for (uint32_t r = 0; r < kBatchRounds; ++r) {
      const unsigned long long base64 = (unsigned long long)tile * kClusterItemTile + wave * (kBatchRounds * 64u) + r * 64u;
      if (base64 >= w_total) break;  // (the whole wave; the rounds behind it start later still)
      const uint32_t base = (uint32_t)base64, word = base >> 6;
      const unsigned long long s = cluster_uniform64(ta.nonempty[word]);
      if (s == 0ull) continue;  // (the whole wave)
      const uint32_t before = (uint32_t)__builtin_amdgcn_readfirstlane((int)(ta.l.list_tiles[word / kClusterListTileWords] + ta.l.word_rank[word]));
      if (before >= ta.l.entry_capacity) continue;  // (the whole wave: every rank of the word is at or above the capacity)
      const uint32_t m0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)ta.l.word_member[word]);
      const ClusterItem it = cluster_list_locate(a, m0, base, lane, w_total, members);
      const uint32_t rank = before + lanes_below(s);
      if (((s >> lane) & 1ull) != 0ull && rank < ta.l.entry_capacity) {  // a set bit is a surviving item: below W
        const unsigned long long mask = ta.triangle_words[base + lane];
        const uint32_t ml = a.lods.bucket_lod[a.bucket[it.inst]];
        const uint32_t mesh = ml >> 3, lod = ml & 7u;
        const MeshChain& ch = a.lods.chain[mesh];
        uint4 e;
        e.x = a.lods.first_instance_base + it.inst;
        e.y = ch.index_offset[lod] + kClusterIndices * it.cluster;  // the source mesh's own range
        e.z = (uint32_t)a.lods.mesh_draw[mesh].vertex_offset;
        e.w = cluster_list_index_count(it.cluster, cluster_level_triangles(ch.index_len[lod]));
        ta.l.entries[rank] = e;
        ta.masks[rank] = mask;
      }
    }
  }
}

}  // namespace mip
