// cluster_triangle_kernel.hpp — per-triangle culling of surviving clusters (mip_cull_cluster_triangles; extension, not reference
// behaviour), gfx950: the per-triangle stage's test (triangle_kernels.hpp: triangle_test, the same device functions) on the
// triangles of every work item mip_cull_clusters' tests let through, the survivors' indices packed into one stream and one
// command per run of surviving clusters into it. include/mi_instance_pipeline.h specifies it, tests/cluster_triangle_restatement.py
// restates it in numpy, cluster_triangle_plan.hpp holds the arithmetic that is not a kernel. Instantiated in api_cluster.hip only.
//
// A call is count -> scan -> members -> cull -> heads of cluster_kernel.hpp, the instantiations mip_cull_clusters launches, and
// behind them, on the same stream:
//
//   test       one wave per survive word, walking the cull kernel's item tiles. A zero word stores its zero total and nothing
//              else. Otherwise the wave locates its 64 items (cluster_locate), lane j forms the model matrix of item j from the
//              instance columns — the sixteen floats mip_run writes — and the wave walks the word's set bits: the matrix of the
//              item is broadcast to scalar registers, lane t loads the index triple and the three positions of triangle t of the
//              cluster through bounded descriptors and runs triangle_test; the ballot is the item's 8-byte TRIANGLE WORD. The
//              word's surviving triangles -> word_total; the tile's surviving and tested triangles -> tile_kept / tile_tested
//   scan       one workgroup, in the epilogue's place: the head counts and the tiles' surviving triangles become exclusive
//              prefixes; the totals; whether the index stream fits (cluster_triangle_index_fits) — if not, the kernels behind
//              see W = 0; cmd_count, the six stats, the overflow status
//   write      one wave per survive word again: the exclusive prefix of every item (4 bytes, with an entry at W) from the tile's
//              prefix, the totals of the tile's words in front and a wave scan of the items' popcounts; then, per surviving
//              item, lane t copies the index triple of a surviving triangle t to 3 x (prefix + set bits below t). Indices are
//              read again; no vertex is, and nothing is computed
//   commands   mip_cull_clusters' heads, ranks and runs; indexCount and firstIndex from the item prefix at the head and behind
//              the run
//
// No workgroup waits for another and nothing depends on the order workgroups start in; the three looping grids take
// cluster_permute_tile in the diagnostic build.
#pragma once

#include "cluster_kernel.hpp"
#include "cluster_triangle_plan.hpp"
#define MIP_TRIANGLE_DEVICE_HELPERS_ONLY  // triangle_test, model_is_affine, times12; the stage's kernels stay in stages_tu.hip
#include "triangle_kernels.hpp"

#pragma clang fp contract(off)

namespace mip {

static_assert(kClusterTriangleTileWords == kWaves * kBatchRounds, "a tile of the test / write kernels is the cull kernel's: a word per wave and round");

// tri_scalars[]: what the triangle scan leaves for the write and the commands kernel
constexpr uint32_t kClusterTriScW = 0;      // W, or 0 when the call writes no stream (it does not run, or its indices do not fit)
constexpr uint32_t kClusterTriScWords = 1;

struct ClusterTriangleArgs {
  ClusterArgs c;                    // mip_cull_clusters' block, as its five kernels in front take it
  const float* vertices;
  const uint32_t* indices;
  unsigned long long vertex_bytes;  // the uploaded positions (read through a bounded descriptor)
  uint32_t geometry_finite;         // every uploaded position is finite: an affine matrix may take triangle_test<true>
  float pv[16];                     // the frame's
  // scratch
  unsigned long long* triangle_words;  // per work item (written for the surviving ones only)
  uint32_t* item_prefix;            // W + 1
  uint32_t* word_total;             // per survive word: surviving triangles of its items
  uint32_t* tile_kept;              // per item tile: surviving triangles; the scan makes them exclusive prefixes
  uint32_t* tile_tested;
  uint32_t* tri_scalars;            // kClusterTriScWords
  // outputs
  uint32_t* culled_indices;
  uint32_t index_capacity;
};

__device__ __forceinline__ unsigned long long cluster_uniform64(unsigned long long v) {
  return ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32) |
         (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}
__device__ __forceinline__ uint32_t cluster_lane_word(uint32_t v, uint32_t k) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)k); }
__device__ __forceinline__ float cluster_lane_word(float v, uint32_t k) { return __uint_as_float(cluster_lane_word(__float_as_uint(v), k)); }

// The model matrix of instance i as mip_run stores it (store_piece): rows 0..2 from the finite form when every input of the
// WAVE's instances is finite, else from the literal chain (for finite inputs the two agree as numbers: instance_tiered takes
// either, by the wave); row 3 is (0, 0, 0, 1), NaN where the literal chain made it NaN.
__device__ __forceinline__ void cluster_item_model(const ClusterArgs& a, uint32_t i, float (&model)[16]) {
  const float px = a.lods.pos[3 * (size_t)i + 0], py = a.lods.pos[3 * (size_t)i + 1], pz = a.lods.pos[3 * (size_t)i + 2];
  const float4 q = a.lods.rot[i];
  const float sc = a.lods.scale[i];
  float rm[3][3];
  quat_to_rotation(q.x, q.y, q.z, q.w, rm);
  Instance inst;
  if (__builtin_expect(__any(!(finite_magnitude(rm, px, py, pz, sc) < kFiniteLimit)), 0)) {
    float m[16];
    model_general(rm, px, py, pz, sc, inst, m);
  } else {
    model_fast(rm, px, py, pz, sc, inst);
  }
#pragma unroll
  for (uint32_t c = 0; c < 4; ++c) {
#pragma unroll
    for (uint32_t r = 0; r < 3; ++r) model[c * 4 + r] = inst.m[c * 3 + r];
    model[c * 4 + 3] = ((inst.row3 >> c) & 1u) ? __uint_as_float(0x7fc00000u) : (c == 3u ? 1.0f : 0.0f);
  }
}

// The level a work item's cluster is cut from: where its triangles start in the index buffer, how many it holds, the mesh's
// vertex offset (>= 0: mip_build_clusters checked every level).
struct ClusterSource {
  uint32_t first_index, triangles, vertex_offset;
};
__device__ __forceinline__ ClusterSource cluster_source(const ClusterArgs& a, const ClusterItem& it) {
  const uint32_t ml = a.lods.bucket_lod[a.bucket[it.inst]];
  const uint32_t mesh = ml >> 3, lod = ml & 7u;
  const MeshChain& ch = a.lods.chain[mesh];
  return {ch.index_offset[lod] + kClusterIndices * it.cluster, cluster_triangles(it.cluster, cluster_level_triangles(ch.index_len[lod])),
          (uint32_t)a.lods.mesh_draw[mesh].vertex_offset};
}

// test: the triangle word of every surviving item; the totals of every word and tile
__global__ __launch_bounds__(kClusterThreads, 4) void mip_cluster_triangle_test_kernel(const ClusterTriangleArgs ta) {
  __shared__ uint32_t s_kept[kWaves], s_tested[kWaves];
  const ClusterArgs& a = ta.c;
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
      const uint32_t base = (uint32_t)base64;
      const unsigned long long survive = cluster_uniform64(a.words[base >> 6].x);
      uint32_t word_kept = 0;
      if (survive != 0ull) {  // (the whole wave)
        const ClusterItem it = cluster_locate(a, base, lane, w_total, members);
        float mine[16];
        cluster_item_model(a, it.inst, mine);
        const ClusterSource src = cluster_source(a, it);
        // The walk is the per-triangle stage's pipeline (chunk_walk): the index triple of the NEXT item is in flight under this
        // item's gathers and test, and no memory operation stands in a branch; the last item reads its own triple again (in
        // bounds, never used). Lane k keeps the triangle word of item k: one store of the whole word's words behind the walk.
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
          word_kept += (uint32_t)__popcll(mask);
          tested += tris;
          k = k_next;
        }
        if (((survive >> lane) & 1ull) != 0ull) ta.triangle_words[base + lane] = mine_word;
      }
      if (lane == 0u) ta.word_total[base >> 6] = word_kept;
      kept += word_kept;
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

// scan, in the epilogue's place: the head counts and the tiles' surviving triangles become exclusive prefixes; the count, the
// stats and the status of the call; whether the kernels behind it write. One workgroup.
static __global__ __launch_bounds__(kClusterThreads) __attribute__((unused)) void mip_cluster_triangle_scan_kernel(const ClusterTriangleArgs ta) {
  __shared__ uint32_t s_wave[kWaves];
  __shared__ unsigned long long s_scan[kClusterThreads];
  const ClusterArgs& a = ta.c;
  const uint32_t w_total = a.scalars[kClusterScW];  // 0 when the call does not run
  const uint32_t head_tiles = cluster_head_tiles(w_total), item_tiles = cluster_item_tiles(w_total);
  uint32_t heads_before = 0, survivors = 0;
  for (uint32_t first = 0; first < head_tiles; first += kClusterThreads) {
    const uint32_t t = first + threadIdx.x;
    uint32_t th, ts;
    const uint32_t excl = batch_block_scan(t < head_tiles ? a.tile_heads[t] : 0u, s_wave, th);
    (void)batch_block_scan(t < head_tiles ? a.tile_survivors[t] : 0u, s_wave, ts);
    if (t < head_tiles) a.tile_heads[t] = heads_before + excl;
    heads_before += th;
    survivors += ts;
  }
  unsigned long long kept_before = 0, tested = 0;
  for (uint32_t first = 0; first < item_tiles; first += kClusterThreads) {
    const uint32_t t = first + threadIdx.x;
    unsigned long long tk, tt;
    const unsigned long long excl = cluster_block_scan64(t < item_tiles ? ta.tile_kept[t] : 0u, s_scan, tk);
    (void)cluster_block_scan64(t < item_tiles ? ta.tile_tested[t] : 0u, s_scan, tt);
    if (t < item_tiles) ta.tile_kept[t] = (uint32_t)(kept_before + excl);  // (exact whenever the stream fits: only then is it read)
    kept_before += tk;
    tested += tt;
  }
  if (threadIdx.x == 0u) {
    const bool fits = cluster_triangle_index_fits(kept_before, ta.index_capacity);
    ta.tri_scalars[kClusterTriScW] = fits ? w_total : 0u;
    *a.cmd_count = !fits ? 0u : heads_before < a.cmd_capacity ? heads_before : a.cmd_capacity;
    if (a.stats) {
      a.stats[0] = heads_before;
      a.stats[1] = survivors;
      a.stats[2] = a.scalars[kClusterScWTrue];
      a.stats[3] = a.scalars[kClusterScMembers];
      a.stats[4] = (uint32_t)kept_before;
      a.stats[5] = (uint32_t)tested;
    }
    if (!fits || heads_before > a.cmd_capacity) cluster_raise(a, kClusterStatusCapacity);
  }
}

// write: every item's exclusive prefix; the surviving triangles' indices to their places in the stream
__global__ __launch_bounds__(kClusterThreads) void mip_cluster_triangle_write_kernel(const ClusterTriangleArgs ta) {
  const ClusterArgs& a = ta.c;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t w_total = ta.tri_scalars[kClusterTriScW], members = a.scalars[kClusterScMembers];
  const uint32_t n_tiles = cluster_item_tiles(w_total), n_words = cluster_survive_words(w_total);
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t tile = cluster_loop_tile(a, t, n_tiles);
    // the totals of the tile's words, one per lane: lane w holds the triangles of the words in front of word w
    const uint32_t word = tile * kClusterTriangleTileWords + lane;  // (tile < 2^22: no wrap)
    const uint32_t total = lane < kClusterTriangleTileWords && word < n_words ? ta.word_total[word] : 0u;
    const uint32_t words_before = wave_inclusive_scan(total) - total;
    const uint32_t tile_before = ta.tile_kept[tile];
#pragma unroll 1
    for (uint32_t r = 0; r < kBatchRounds; ++r) {
      const unsigned long long base64 = (unsigned long long)tile * kClusterItemTile + wave * (kBatchRounds * 64u) + r * 64u;
      if (base64 >= w_total) break;  // (the whole wave; the rounds behind it start later still)
      const uint32_t base = (uint32_t)base64;
      const unsigned long long survive = cluster_uniform64(a.words[base >> 6].x);
      const bool active = base + lane < w_total;  // (base <= 2^32 - 64: the sum does not wrap)
      const unsigned long long mine = ((survive >> lane) & 1ull) != 0ull ? ta.triangle_words[base + lane] : 0ull;  // a surviving item is below W
      const uint32_t count = (uint32_t)__popcll(mine);
      const uint32_t prefix = tile_before + cluster_lane_word(words_before, wave * kBatchRounds + r) + wave_inclusive_scan(count) - count;
      if (active) ta.item_prefix[base + lane] = prefix;
      if (base + lane == w_total - 1u) ta.item_prefix[w_total] = prefix + count;
      if (survive == 0ull) continue;  // (the whole wave)
      const ClusterItem it = cluster_locate(a, base, lane, w_total, members);
      const ClusterSource src = cluster_source(a, it);
      for (unsigned long long rest = survive; rest != 0ull; rest &= rest - 1ull) {
        const uint32_t k = (uint32_t)__builtin_ctzll(rest);
        const unsigned long long mask = ((unsigned long long)cluster_lane_word((uint32_t)(mine >> 32), k) << 32) | cluster_lane_word((uint32_t)mine, k);
        const uint32_t first_index = cluster_lane_word(src.first_index, k), before = cluster_lane_word(prefix, k);
        if (((mask >> lane) & 1ull) != 0ull) {  // triangle `lane` of the cluster: below its triangle count
          const uint32_t* in = ta.indices + (size_t)first_index + 3u * lane;
          uint32_t* o = ta.culled_indices + 3u * ((size_t)before + lanes_below(mask));  // within index_capacity: the scan decided
          o[0] = in[0];
          o[1] = in[1];
          o[2] = in[2];
        }
      }
    }
  }
}

// commands: mip_cull_clusters' heads, ranks and runs into the culled stream. mip_cluster_commands_kernel's lines with another W
// and another indexCount / firstIndex: sharing one body between the two moved an instruction of the kernel mip_cull_clusters
// launches, which is held to the instructions it had (DESIGN sections 25, 27 and 28).
static __global__ __launch_bounds__(kClusterThreads) __attribute__((unused)) void mip_cluster_triangle_commands_kernel(const ClusterTriangleArgs ta) {
  __shared__ uint32_t s_wave[kWaves];
  __shared__ uint32_t s_rank[kClusterHeadTileWords];
  __shared__ unsigned long long s_mask[kClusterHeadTileWords];
  const ClusterArgs& a = ta.c;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t w_total = ta.tri_scalars[kClusterTriScW], members = a.scalars[kClusterScMembers];
  const uint32_t n_words = cluster_survive_words(w_total), n_tiles = cluster_head_tiles(w_total);
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t tile = cluster_loop_tile(a, t, n_tiles);
    {
      const uint32_t word = tile * kClusterHeadTileWords + threadIdx.x;
      const unsigned long long mask = word < n_words ? cluster_head_mask(a, word) : 0ull;
      uint32_t unused_total;
      const uint32_t excl = batch_block_scan((uint32_t)__popcll(mask), s_wave, unused_total);
      s_rank[threadIdx.x] = a.tile_heads[tile] + excl;  // the heads in front of this word (the scan: the tiles before)
      s_mask[threadIdx.x] = mask;
    }
    __syncthreads();
#pragma unroll 1
    for (uint32_t j = 0; j < 64u; ++j) {
      const uint32_t local = wave * 64u + j;
      const unsigned long long mask = cluster_uniform64(s_mask[local]);
      if (mask == 0ull) continue;  // (the whole wave)
      const uint32_t base = (tile * kClusterHeadTileWords + local) * 64u;  // < W: the word holds a survivor
      const ClusterItem it = cluster_locate(a, base, lane, w_total, members);
      const uint32_t rank = s_rank[local] + lanes_below(mask);
      if (((mask >> lane) & 1ull) != 0ull && rank < a.cmd_capacity) {
        const uint32_t ml = a.lods.bucket_lod[a.bucket[it.inst]];
        const uint32_t mesh = ml >> 3, lod = ml & 7u;
        const uint32_t limit = cluster_level_clusters(a.lods.chain[mesh].index_len[lod]) - it.cluster;  // clusters the instance has left, this one included
        // the run: this survivor and the survivors straight behind it, inside the instance
        uint32_t run = 0, at = base + lane;
        while (run < limit) {
          const uint32_t bit = at & 63u, room = 64u - bit;
          const unsigned long long rest = ~(a.words[at >> 6].x >> bit);  // the shift brings zeros in: a clear bit below `room`, unless bit == 0
          const uint32_t ones = rest ? (uint32_t)__builtin_ctzll(rest) : 64u;
          const uint32_t take = ones < limit - run ? ones : limit - run;
          run += take;
          at += take;
          if (ones < room) break;  // a cluster that does not survive ends the run
        }
        const uint32_t first = ta.item_prefix[base + lane];
        uint32_t* o = a.cmds + (size_t)rank * kCmdWords;
        o[0] = 3u * (ta.item_prefix[at] - first);  // (at = the item behind the run, <= W)
        o[1] = 1u;
        o[2] = 3u * first;
        o[3] = (uint32_t)a.lods.mesh_draw[mesh].vertex_offset;
        o[4] = a.lods.first_instance_base + it.inst;
      }
    }
    __syncthreads();  // s_rank / s_mask are free for the next tile
  }
}

}  // namespace mip
